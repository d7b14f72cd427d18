// Locating cut-outs in the original before tracing them (ssw_locate_rgb8): a search for a translation.  For every position of
// the (restored) suspect R inside the original O the integer luma difference is summed, the 8 best positions of a coarse
// search are rescored at full resolution, and the best of those is the answer.  include/ssw.h states the definition; every
// quantity is an integer, so nothing here depends on the order of a sum and the result equals the numpy restatement of
// tests/test_locate_cpu.py exactly.  The reference has no counterpart (tests/attack_crop.rs:56-70 knows where its crop lies).
//
// Kernels:
//   locate_strip_alpha_kernel   RGBA -> RGB in front of a resize (the search ignores alpha)                       HBM-bound
//   locate_luma_kernel          RGB / RGBA u8 -> u8 luma plane, L = (77 R + 150 G + 29 B + 128) >> 8             HBM-bound
//   locate_box_kernel           4 x 4 box means of a luma plane: the 16 phase planes [y mod 4][x mod 4][H/4][W/4] of the
//                               original (the box at EVERY pixel, not decimated), the decimated plane S_f of a suspect
//   locate_coarse_kernel        THE HOT PATH: D(x, y) = sum |T - plane window| for a tile of 64 x 32 positions of one plane
//                               (a phase plane against S_f when f = 4, L_O against L_R when f = 1): rows of both staged in
//                               LDS, a lane owns one x and eight y, forms its 4-byte windows with v_alignbyte_b32 and sums
//                               four pixels per v_sad_u8
//   locate_topk_kernel          round r of 8: the minimum of the keys (D << 32) | (y nx + x) above round r - 1's -- a u64
//                               minimum per block, then one atomic minimum: deterministic, ties to the lower (y, x)
//   locate_fine_kernel          full-resolution SAD of one (suspect, candidate) per block group, u64
//   locate_final_kernel         the candidate with the smallest (SAD, y, x)
// Launch descriptors travel as kernel arguments, 32 suspects per launch, like restore.hip's.
//
// The scale ladder (ssw_locate_scaled_rgb8) for cut-outs whose size is not known either adds
//   locate_box8_kernel          8 x 8 box means of the original at every fourth position, as 2 x 2 phase planes
//   locate_rung_kernel          THE LADDER'S HOT PATH: one (suspect, rung) -- the fused CatmullRom tile of resize_common.hpp
//                               (resize_tile_front) whose epilogue is the horizontal pass, clamp + round, luma and the 8 x 8 box
//                               sum; only the box means T_j are stored
// and reuses locate_coarse_kernel (f = 2) and round 0 of locate_topk_kernel per rung; the 8 best rungs are refined by windowed
// searches of the kernels above (a base offset in their descriptors).  The rungs are chosen on the host.
#include <algorithm>
#include <atomic>
#include <vector>

#include <cstring>
#include <map>

#include "resize_common.hpp"
#include "ssw_host.hpp"

namespace ssw {

constexpr unsigned LOC_BATCH = 32;
constexpr unsigned LOC_TOP = 8;               // candidates that are rescored at full resolution
constexpr unsigned LOC_TX = 64, LOC_TY = 32;  // candidate positions of one block of the coarse kernel
constexpr unsigned LOC_YPL = 8;               // y positions per lane
constexpr unsigned LOC_JB = 8;                // template rows per LDS chunk
constexpr unsigned LOC_KW = 16;               // template words (4 pixels each) per LDS chunk
constexpr unsigned LOC_PROWS = LOC_TY + LOC_JB - 1;
constexpr unsigned LOC_PWORDS = LOC_TX / 4 + LOC_KW;      // the last window of lane 63 ends in word 15 + 15 + 1
constexpr uint64_t LOC_NONE = ~0ull;

struct LumaDev { const uint8_t* src; uint8_t* out; uint32_t w, h, c, pitch; };
struct LumaBatch { LumaDev it[LOC_BATCH]; };
struct BoxDev { const uint8_t* luma; uint8_t* out; uint32_t lpitch, w, h, opitch, nxq, nyq, phases, plane_stride; };
struct BoxBatch { BoxDev it[LOC_BATCH]; };
struct CoarseDev {
    const uint8_t* plane;        // phase plane 0 (f = 4) or L_O (f = 1)
    const uint8_t* tmpl;         // S_f (f = 4) or L_R (f = 1)
    uint32_t* D;                 // [ny][nx]
    uint32_t ppitch, prows, plane_stride;
    uint32_t tpitch, tw, th;
    uint32_t nx, ny, f;          // f = 2: the scale ladder -- 2 x 2 phase planes of the 4-decimated 8 x 8 box plane
    uint32_t tiles_x, tiles_y, tile_begin;
    uint32_t bxw, by;            // a windowed search: the plane word and row of candidate (0, 0); 0 for a search of the whole frame
};
struct CoarseBatch { CoarseDev it[LOC_BATCH]; };
struct TopDev { const uint32_t* D; uint32_t n, nx, skipx, skipy; };     // skipx / skipy (with nx): candidates left of / above these are not part of the window
struct TopBatch { TopDev it[LOC_BATCH]; };
struct FineDev { const uint8_t* lr; uint32_t rpitch, pw, ph, nx, bx, by; };   // bx, by: the frame position of candidate (0, 0)
struct FineBatch { FineDev it[LOC_BATCH]; };

__device__ inline uint32_t locate_luma(uint32_t r, uint32_t g, uint32_t b) { return (77u * r + 150u * g + 29u * b + 128u) >> 8; }

// One thread = one pixel.  grid: (pixels / 256)
__global__ __launch_bounds__(256) void locate_strip_alpha_kernel(const uint8_t* __restrict__ in, size_t npix, uint8_t* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= npix) return;
    out[3 * i] = in[4 * i]; out[3 * i + 1] = in[4 * i + 1]; out[3 * i + 2] = in[4 * i + 2];
}

// One thread = 4 consecutive pixels of a row = one 32-bit word of the luma plane (pitch % 4 == 0; bytes past w are 0).
// grid: (words of the widest row / 256, rows, images).  No alignment is assumed of the source.
__global__ __launch_bounds__(256) void locate_luma_kernel(LumaBatch b) {
    const LumaDev& d = b.it[blockIdx.z];
    const unsigned wd = blockIdx.x * 256 + threadIdx.x;
    if (4 * wd >= d.pitch) return;
    for (unsigned row = blockIdx.y; row < d.h; row += gridDim.y) {
        const uint8_t* __restrict__ s = d.src + ((size_t)row * d.w + 4 * wd) * d.c;
        uint32_t v = 0;
#pragma unroll
        for (unsigned p = 0; p < 4; ++p)
            if (4 * wd + p < d.w) v |= locate_luma(s[p * d.c], s[p * d.c + 1], s[p * d.c + 2]) << (8 * p);
        *reinterpret_cast<uint32_t*>(d.out + (size_t)row * d.pitch + 4 * wd) = v;
    }
}

// One thread = one byte of an output plane: out[z][yq][xq] = (sum of the 4 x 4 lumas at (4 xq + z % 4, 4 yq + z / 4) + 8) >> 4
// where that box lies inside the plane and xq < nxq, 0 elsewhere (the pitch's padding included).  grid: (opitch / 256, nyq, images)
__global__ __launch_bounds__(256) void locate_box_kernel(BoxBatch b) {
    const BoxDev& d = b.it[blockIdx.z];
    const unsigned xq = blockIdx.x * 256 + threadIdx.x;
    if (xq >= d.opitch) return;
    for (unsigned z = 0; z < d.phases; ++z) {
        const unsigned px = z & 3, py = z >> 2;
        for (unsigned yq = blockIdx.y; yq < d.nyq; yq += gridDim.y) {
            const unsigned x = 4 * xq + px, y = 4 * yq + py;
            uint32_t v = 0;
            if (xq < d.nxq && x + 4 <= d.w && y + 4 <= d.h) {
                uint32_t s = 8;
#pragma unroll
                for (unsigned j = 0; j < 4; ++j) {
                    const uint8_t* __restrict__ r = d.luma + (size_t)(y + j) * d.lpitch + x;
                    s += (uint32_t)r[0] + r[1] + r[2] + r[3];
                }
                v = s >> 4;
            }
            d.out[(size_t)z * d.plane_stride + (size_t)yq * d.opitch + xq] = (uint8_t)v;
        }
    }
}

// The inner loop of the coarse kernel over one LDS chunk: LOC_JB template rows x LOC_KW template words against the plane
// rows a wave's eight y positions need.  A plane row's window is formed once per word (one ds_read + one v_alignbyte_b32)
// and used by every (y, j) pair that meets it: 64 v_sad_u8 for 15 windows and 8 template words.  MASKED: the chunk holds
// the template's right or bottom edge -- the bytes past tw are masked out of both operands and rows past th are skipped.
template <bool MASKED>
__device__ inline void locate_chunk(const uint32_t (*sP)[LOC_PWORDS], const uint32_t (*sT)[LOC_KW], unsigned yb, unsigned wl, unsigned sh,
                                    int cols_left, unsigned rows_left, uint32_t (&acc)[LOC_YPL]) {
    constexpr unsigned NR = LOC_YPL + LOC_JB - 1;
    uint32_t prev[NR];
#pragma unroll
    for (unsigned r = 0; r < NR; ++r) prev[r] = sP[yb + r][wl];
#pragma unroll 2
    for (unsigned k = 0; k < LOC_KW; ++k) {
        uint32_t mask = 0xFFFFFFFFu;
        if (MASKED) {
            const int rem = cols_left - 4 * (int)k;                 // template bytes from this word on (uniform)
            if (rem <= 0) break;
            if (rem < 4) mask = (1u << (8 * rem)) - 1u;
        }
        uint32_t t[LOC_JB];
#pragma unroll
        for (unsigned j = 0; j < LOC_JB; ++j) t[j] = sT[j][k] & mask;
#pragma unroll
        for (unsigned r = 0; r < NR; ++r) {
            const uint32_t cur = sP[yb + r][wl + k + 1];
            const uint32_t win = __builtin_amdgcn_alignbyte(cur, prev[r], sh) & mask;
            prev[r] = cur;
#pragma unroll
            for (unsigned j = 0; j < LOC_JB; ++j) {
                if (j > r || r - j >= LOC_YPL) continue;            // compile-time: y = r - j is one of the lane's eight
                if (MASKED && j >= rows_left) continue;             // uniform
                acc[r - j] = __builtin_amdgcn_sad_u8(win, t[j], acc[r - j]);
            }
        }
    }
}

// One block = 64 x 32 candidate positions of one plane of one suspect; wave v owns the y positions 8 v .. 8 v + 7, lane l the
// x position l.  grid: (tiles of all suspects of the launch).  LDS: 39 plane rows of 32 words + 8 template rows of 16 words
// (5.5 KB) per chunk; reads outside the plane or the template are staged as 0 and only ever reach positions that are not
// candidates, which are not written.
__global__ __launch_bounds__(256) void locate_coarse_kernel(CoarseBatch b, unsigned n) {
    __shared__ uint32_t sP[LOC_PROWS][LOC_PWORDS];
    __shared__ uint32_t sT[LOC_JB][LOC_KW];
    unsigned s = 0;
    while (s + 1 < n && blockIdx.x >= b.it[s + 1].tile_begin) ++s;
    const CoarseDev& d = b.it[s];
    const unsigned tile = blockIdx.x - d.tile_begin;
    const unsigned per_phase = d.tiles_x * d.tiles_y;
    const unsigned phase = tile / per_phase, tp = tile - phase * per_phase;
    const unsigned px = phase % d.f, py = phase / d.f;
    const unsigned nxp = d.nx > px ? (d.nx - px + d.f - 1) / d.f : 0;      // candidates of this phase
    const unsigned nyp = d.ny > py ? (d.ny - py + d.f - 1) / d.f : 0;
    const unsigned x0 = (tp % d.tiles_x) * LOC_TX, y0 = (tp / d.tiles_x) * LOC_TY;
    if (x0 >= nxp || y0 >= nyp) return;
    const uint32_t* __restrict__ plane = reinterpret_cast<const uint32_t*>(d.plane + (size_t)phase * d.plane_stride);
    const uint32_t* __restrict__ tmpl = reinterpret_cast<const uint32_t*>(d.tmpl);
    const unsigned pwords = d.ppitch / 4, twords = d.tpitch / 4;
    const unsigned tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned yb = wave * LOC_YPL, wl = lane >> 2, sh = lane & 3;
    uint32_t acc[LOC_YPL];
#pragma unroll
    for (unsigned y = 0; y < LOC_YPL; ++y) acc[y] = 0;
    for (unsigned j0 = 0; j0 < d.th; j0 += LOC_JB) {
        for (unsigned i0 = 0; i0 < d.tw; i0 += 4 * LOC_KW) {
            __syncthreads();
            for (unsigned it = tid; it < LOC_PROWS * LOC_PWORDS; it += 256) {
                const unsigned r = it / LOC_PWORDS, c = it - r * LOC_PWORDS;
                const unsigned row = d.by + y0 + j0 + r, wd = d.bxw + (x0 + i0) / 4 + c;
                sP[r][c] = (row < d.prows && wd < pwords) ? plane[(size_t)row * pwords + wd] : 0u;
            }
            if (tid < LOC_JB * LOC_KW) {
                const unsigned j = tid / LOC_KW, k = tid - j * LOC_KW;
                const unsigned row = j0 + j, wd = i0 / 4 + k;
                sT[j][k] = (row < d.th && wd < twords) ? tmpl[(size_t)row * twords + wd] : 0u;
            }
            __syncthreads();
            if (d.tw - i0 >= 4 * LOC_KW && d.th - j0 >= LOC_JB) locate_chunk<false>(sP, sT, yb, wl, sh, 0, 0, acc);
            else locate_chunk<true>(sP, sT, yb, wl, sh, (int)(d.tw - i0), d.th - j0, acc);
        }
    }
    const unsigned xq = x0 + lane;
    if (xq >= nxp) return;
#pragma unroll
    for (unsigned y = 0; y < LOC_YPL; ++y) {
        const unsigned yq = y0 + yb + y;
        if (yq < nyp) d.D[(size_t)(yq * d.f + py) * d.nx + (xq * d.f + px)] = acc[y];
    }
}

__device__ inline uint64_t locate_block_min(uint64_t m, uint64_t* s_red) {
#pragma unroll
    for (int o = 32; o; o >>= 1) { const uint64_t v = __shfl_down(m, o); m = v < m ? v : m; }
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0)
        for (unsigned w = 1; w < 4; ++w) m = s_red[w] < m ? s_red[w] : m;
    return m;                                          // valid in thread 0
}
__device__ inline uint64_t locate_block_sum(uint64_t m, uint64_t* s_red) {
#pragma unroll
    for (int o = 32; o; o >>= 1) m += __shfl_down(m, o);
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) m = s_red[0] + s_red[1] + s_red[2] + s_red[3];
    return m;
}

// keys: [suspect][LOC_TOP] u64, all LOC_NONE before round 0.  grid: (blocks, suspects)
__global__ __launch_bounds__(256) void locate_topk_kernel(TopBatch b, uint64_t* __restrict__ keys, unsigned round) {
    __shared__ uint64_t s_red[4];
    const TopDev& d = b.it[blockIdx.y];
    uint64_t* k = keys + (size_t)blockIdx.y * LOC_TOP;
    const uint64_t prev = round ? k[round - 1] : 0;
    if (round && prev == LOC_NONE) return;             // fewer positions than rounds (uniform)
    uint64_t m = LOC_NONE;
    for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < d.n; i += gridDim.x * 256) {
        const uint64_t key = ((uint64_t)d.D[i] << 32) | i;
        if ((d.skipx | d.skipy) && (i % d.nx < d.skipx || i / d.nx < d.skipy)) continue;
        if ((!round || key > prev) && key < m) m = key;
    }
    m = locate_block_min(m, s_red);
    if (threadIdx.x == 0 && m != LOC_NONE) atomicMin(reinterpret_cast<unsigned long long*>(k + round), (unsigned long long)m);
}

// grid: (row groups, LOC_TOP, suspects); sums [suspect][LOC_TOP] u64, zero before the launch.  lo: the original's luma plane
// (opitch % 4 == 0, 16 bytes of slack behind its last row).
__global__ __launch_bounds__(256) void locate_fine_kernel(FineBatch b, const uint8_t* __restrict__ lo, unsigned opitch,
                                                          const uint64_t* __restrict__ keys, uint64_t* __restrict__ sums) {
    __shared__ uint64_t s_red[4];
    const FineDev& d = b.it[blockIdx.z];
    const uint64_t key = keys[(size_t)blockIdx.z * LOC_TOP + blockIdx.y];
    if (key == LOC_NONE) return;
    const uint32_t idx = (uint32_t)key, y = d.by + idx / d.nx, x = d.bx + idx % d.nx;
    const uint32_t* __restrict__ lo32 = reinterpret_cast<const uint32_t*>(lo);
    uint64_t total = 0;
    for (unsigned j = blockIdx.x; j < d.ph; j += gridDim.x) {
        const uint32_t* __restrict__ r32 = reinterpret_cast<const uint32_t*>(d.lr + (size_t)j * d.rpitch);
        uint32_t acc = 0;
        for (unsigned i = threadIdx.x; 4 * i < d.pw; i += 256) {
            const size_t a = (size_t)(y + j) * opitch + x + 4 * i;
            const uint32_t w0 = lo32[a >> 2], w1 = lo32[(a >> 2) + 1];
            const unsigned rem = d.pw - 4 * i;
            const uint32_t mask = rem >= 4 ? 0xFFFFFFFFu : (1u << (8 * rem)) - 1u;
            acc = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(w1, w0, (uint32_t)(a & 3)) & mask, r32[i] & mask, acc);
        }
        total += acc;
    }
    total = locate_block_sum(total, s_red);
    if (threadIdx.x == 0 && total) atomicAdd(reinterpret_cast<unsigned long long*>(sums + (size_t)blockIdx.z * LOC_TOP + blockIdx.y), (unsigned long long)total);
}

// One thread per suspect: res[2 s] = SAD, res[2 s + 1] = (y << 32) | x of the candidate with the smallest (SAD, y, x)
__global__ __launch_bounds__(64) void locate_final_kernel(FineBatch b, unsigned n, const uint64_t* __restrict__ keys,
                                                          const uint64_t* __restrict__ sums, uint64_t* __restrict__ res) {
    const unsigned s = blockIdx.x * 64 + threadIdx.x;
    if (s >= n) return;
    uint64_t best = LOC_NONE;
    uint32_t best_idx = 0xFFFFFFFFu;
    for (unsigned t = 0; t < LOC_TOP; ++t) {
        const uint64_t key = keys[(size_t)s * LOC_TOP + t];
        if (key == LOC_NONE) break;
        const uint64_t sad = sums[(size_t)s * LOC_TOP + t];
        const uint32_t idx = (uint32_t)key;
        if (sad < best || (sad == best && idx < best_idx)) { best = sad; best_idx = idx; }
    }
    const uint32_t y = b.it[s].by + best_idx / b.it[s].nx, x = b.it[s].bx + best_idx % b.it[s].nx;
    res[2 * s] = best;
    res[2 * s + 1] = ((uint64_t)y << 32) | x;
}

// ---- the scale ladder (ssw_locate_scaled_rgb8) --------------------------------------------------------------------------------
// One (suspect, rung) of a launch: the suspect resized to pw x ph, of which only the 8 x 8 box means T [th][tw] are stored.
struct RungDev {
    const uint8_t* src;          // the suspect [sh][sw][C]
    uint8_t* T;                  // [th][tpitch]
    ResizeTapPtrs taps;          // tables in the one buffer of the call
    ResizeTile tl;               // oyb, oxb multiples of 8: no box straddles two blocks
    uint32_t sw;
    uint32_t ow, oh;             // 8 tw, 8 th: the output pixels that lie in a box
    uint32_t tpitch;
    uint32_t tile_begin;
};
struct RungBatch { RungDev it[LOC_BATCH]; };

// One thread = one byte of a phase plane: out[z][yq][xq] = (sum of the 8 x 8 lumas at (4 (2 xq + z % 2), 4 (2 yq + z / 2)) + 32) >> 6
// where that box lies inside the plane, 0 elsewhere (the pitch's padding included).  grid: (opitch / 256, rows)
__global__ __launch_bounds__(256) void locate_box8_kernel(const uint8_t* __restrict__ luma, unsigned lpitch, unsigned w, unsigned h,
                                                          uint8_t* __restrict__ out, unsigned opitch, unsigned rows, unsigned plane_stride) {
    const unsigned xq = blockIdx.x * 256 + threadIdx.x;
    if (xq >= opitch) return;
    for (unsigned z = 0; z < 4; ++z) {
        for (unsigned yq = blockIdx.y; yq < rows; yq += gridDim.y) {
            const unsigned x = 4 * (2 * xq + (z & 1)), y = 4 * (2 * yq + (z >> 1));
            uint32_t v = 0;
            if (x + 8 <= w && y + 8 <= h) {
                uint32_t s = 32;
#pragma unroll
                for (unsigned j = 0; j < 8; ++j) {
                    const uint32_t* __restrict__ r = reinterpret_cast<const uint32_t*>(luma + (size_t)(y + j) * lpitch + x);   // x, lpitch: multiples of 4
                    s = __builtin_amdgcn_sad_u8(r[0], 0u, s);
                    s = __builtin_amdgcn_sad_u8(r[1], 0u, s);
                }
                v = s >> 6;
            }
            out[(size_t)z * plane_stride + (size_t)yq * opitch + xq] = (uint8_t)v;
        }
    }
}

// THE HOT PATH of the ladder.  One block = one tile of oyb x oxb pixels of one rung: the fused CatmullRom tile of
// resize_common.hpp (tile -> LDS, vertical pass into an f32 strip), then the horizontal pass with clamp + round, luma and the
// 8 x 8 box sum as its epilogue.  R_j never reaches HBM: only T_j is stored.  C = 4: alpha is read past and ignored.
// grid: (tiles of all rungs of the launch); dynamic LDS: the largest tile's.
template <int C>
__global__ __launch_bounds__(256) void locate_rung_kernel(RungBatch b, unsigned n) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned s = 0;
    while (s + 1 < n && blockIdx.x >= b.it[s + 1].tile_begin) ++s;
    const RungDev& d = b.it[s];
    const ResizeTile& tl = d.tl;
    const ResizeLds l = resize_lds_carve(smem, tl, d.taps.hmax, d.taps.vmax);
    unsigned char* s_lum = l.in;                       // reused after the vertical pass: [oyb][oxb] lumas

    const unsigned tid = threadIdx.x;
    // 1. tap tables and input tile -> LDS, 2. vertical pass; noy, nox: multiples of 8
    const ResizeReach rc = resize_tile_front<C>(l, d.taps, tl, blockIdx.x - d.tile_begin, d.ow, d.oh, d.src, d.sw);
    const unsigned oy0 = rc.oy0, ox0 = rc.ox0, noy = rc.noy, nox = rc.nox, a0 = rc.a0;
    // 3. horizontal pass, clamp + round of the colour channels, luma
    for (unsigned it = tid; it < (noy << tl.oxb_log2); it += 256) {
        const unsigned j = it >> tl.oxb_log2, x = it & ((1u << tl.oxb_log2) - 1);
        if (x >= nox) continue;
        float t[C];
        resize_horizontal_pixel<C>(l.v + j * tl.pitch + (l.lh[x] * C - a0), l.wh + x, l.ch[x], tl.oxb, t);
        s_lum[j * tl.oxb + x] = (unsigned char)locate_luma(resize_to_u8(t[0]), resize_to_u8(t[1]), resize_to_u8(t[2]));
    }
    __syncthreads();
    // 4. the boxes of the tile: one thread each, 16 words
    const unsigned nbx = nox / 8, nby = noy / 8;
    for (unsigned it = tid; it < nbx * nby; it += 256) {
        const unsigned bk = it / nbx, bi = it - bk * nbx;
        uint32_t sum = 32;
#pragma unroll
        for (unsigned j = 0; j < 8; ++j) {
            const uint32_t* r = reinterpret_cast<const uint32_t*>(s_lum + (8 * bk + j) * tl.oxb + 8 * bi);
            sum = __builtin_amdgcn_sad_u8(r[0], 0u, sum);
            sum = __builtin_amdgcn_sad_u8(r[1], 0u, sum);
        }
        d.T[(size_t)(oy0 / 8 + bk) * d.tpitch + ox0 / 8 + bi] = (uint8_t)(sum >> 6);
    }
}

namespace host {

namespace {

size_t up(size_t v, size_t a) { return (v + a - 1) / a * a; }
unsigned grid_rows(size_t rows) { return (unsigned)std::min<size_t>(std::max<size_t>(rows, 1), 65535); }
bool resized(const ssw_placement& p) { return p.pw != p.w || p.ph != p.h; }

// what one suspect needs of the group's workspace, as offsets into it
struct Item {
    size_t index;                 // position in the call
    ssw_placement p;              // normalised, x = y = 0
    unsigned f, nx, ny;           // coarse factor, candidate positions
    unsigned rpitch, tw, th, tpitch;
    size_t off_rgb, off_strip, off_lr, off_sf, off_d, bytes;
    // a windowed search (the refinement of the scale ladder): the frame position of candidate (0, 0) -- aligned down so that
    // plane words and phases line up --, the candidates in front of the window, and whether R is the R of the item before
    unsigned bx = 0, by = 0, skipx = 0, skipy = 0;
    bool share = false;
    size_t bytes_d = 0;
};

constexpr size_t GROUP_BYTES = 256u << 20;      // workspace of one group of suspects (one suspect may need more)

// the original's luma plane, once per call: opitch % 4 == 0, 16 zero bytes of slack behind its last row (locate_fine_kernel)
int original_luma(ssw_ctx* ctx, const uint8_t* dev_base, size_t w, size_t h, uint8_t** lo, unsigned* opitch) {
    *opitch = (unsigned)up(w, 4);
    SSW_TRY(grow_as(ctx->locate.luma, (size_t)*opitch * h + 16, *lo));
    SSW_HIP_CHECK(hipMemsetAsync(*lo + (size_t)*opitch * h, 0, 16, ctx->stream));
    LumaBatch lb{};
    lb.it[0] = LumaDev{dev_base, *lo, (uint32_t)w, (uint32_t)h, 3u, *opitch};
    locate_luma_kernel<<<dim3((*opitch / 4 + 255) / 256, grid_rows(h), 1), 256, 0, ctx->stream>>>(lb);
    SSW_HIP_CHECK(hipGetLastError());
    return SSW_OK;
}

// One search of the coarse kernel: the template tmpl [th][tpitch] over a plane (f = 4: the original's 16 phase planes against
// S_f; f = 2: its 2 x 2 box planes against a rung's T_j; f = 1: L_O against L_R, plane_stride 0), nx x ny candidates into D.
// bx, by: the frame position of candidate (0, 0).  *tiles: the blocks of the launch so far, advanced by this search's.
CoarseDev coarse_desc(const uint8_t* plane, uint32_t ppitch, uint32_t prows, size_t plane_stride, const uint8_t* tmpl, uint32_t tpitch,
                      uint32_t tw, uint32_t th, uint32_t* D, uint32_t nx, uint32_t ny, uint32_t f, uint32_t bx, uint32_t by, unsigned* tiles) {
    const uint32_t tiles_x = ((nx + f - 1) / f + LOC_TX - 1) / LOC_TX, tiles_y = ((ny + f - 1) / f + LOC_TY - 1) / LOC_TY;
    const CoarseDev c{plane, tmpl, D, ppitch, prows, (uint32_t)plane_stride, tpitch, tw, th, nx, ny, f, tiles_x, tiles_y, *tiles, bx / (4 * f), by / f};
    *tiles += tiles_x * tiles_y * f * f;
    return c;
}
unsigned topk_blocks(uint32_t max_n) { return (unsigned)std::min<size_t>(((size_t)max_n + 2047) / 2048, 512); }

// the resize runs on the colour channels alone
int restore_prepare_rgb(ssw_ctx* ctx, std::vector<ssw_placement> pl) {
    for (ssw_placement& p : pl) p.channels = 3;
    return restore_prepare(ctx, pl);
}

// placements (and the windows of a refinement) -> what each search needs; SSW_ERR_UNSUPPORTED: a position is 32 bits of the key
int plan_items(const std::vector<ssw_placement>& pl, const std::vector<LocWindow>* win, size_t w, size_t h, bool luma_planes, std::vector<Item>* items) {
    items->resize(pl.size());
    for (size_t i = 0; i < pl.size(); ++i) {
        Item& it = (*items)[i];
        it.index = i;
        it.p = pl[i];
        it.f = std::min(it.p.pw, it.p.ph) >= 64 ? 4u : 1u;
        it.nx = (unsigned)(w - it.p.pw + 1);
        it.ny = (unsigned)(h - it.p.ph + 1);
        if (win) {
            const LocWindow& wd = (*win)[i];
            const unsigned ax = it.f == 4 ? 16u : 4u, ay = it.f == 4 ? 4u : 1u;
            it.bx = wd.x0 / ax * ax; it.by = wd.y0 / ay * ay;
            it.skipx = wd.x0 - it.bx; it.skipy = wd.y0 - it.by;
            it.nx = wd.x1 - it.bx + 1; it.ny = wd.y1 - it.by + 1;
            it.share = wd.share && i > 0;
        }
        if ((uint64_t)it.nx * it.ny > 0xFFFFFFFFull) return SSW_ERR_UNSUPPORTED;
        it.rpitch = (unsigned)up(it.p.pw, 4);
        it.tw = it.f == 4 ? it.p.pw / 4 : it.p.pw;
        it.th = it.f == 4 ? it.p.ph / 4 : it.p.ph;
        it.tpitch = it.f == 4 ? (unsigned)up(it.tw, 4) : it.rpitch;
        const bool rs = resized(it.p);
        size_t o = 0;
        it.off_rgb = o;   o += rs ? up((size_t)it.p.pw * it.p.ph * 3, 256) : 0;
        it.off_strip = o; o += rs && it.p.channels == 4 ? up((size_t)it.p.w * it.p.h * 3, 256) : 0;
        it.off_lr = o;    o += luma_planes ? 0 : up((size_t)it.rpitch * it.p.ph, 256);      // (a luma plane is read where it lies)
        it.off_sf = o;    o += it.f == 4 ? up((size_t)it.tpitch * it.th, 256) : 0;
        it.bytes_d = up((size_t)it.nx * it.ny * 4, 256);
        it.off_d = o;     o += it.bytes_d;
        it.bytes = o;
    }
    return SSW_OK;
}

// One group: the suspects [g0, g1) in the order of the call, as many as GROUP_BYTES of workspace hold (at least one).  Suspect i
// has its R, luma and S_f at base_off[i - g0] and its D at d_off[i - g0]; a shared R is the one of the item before and lives in
// its group.
struct Group { size_t g0, g1, bytes; std::vector<size_t> base_off, d_off; std::vector<char> shared; };
Group layout_group(const std::vector<Item>& items, size_t g0) {
    Group g{g0, g0, 0, {}, {}, {}};
    auto need = [&](size_t i) { return items[i].share && i > g0 ? items[i].bytes_d : items[i].bytes; };
    while (g.g1 < items.size() && (g.g1 == g0 || g.bytes + need(g.g1) <= GROUP_BYTES)) g.bytes += need(g.g1++);
    for (size_t i = g0, o = 0; i < g.g1; o += need(i++)) {
        const bool sh = items[i].share && i > g0;
        const size_t base = sh ? g.base_off.back() : o;
        g.shared.push_back(sh);
        g.base_off.push_back(base);
        g.d_off.push_back(sh ? o : o + items[i].off_d);
    }
    return g;
}

// the original's planes of a call
struct Original { const uint8_t* lo; unsigned opitch, h; const uint8_t* phases; unsigned qpitch, hq; size_t plane_stride; };

// The searches of the suspects [b0, b0 + m) of a group, m <= LOC_BATCH, whose R (where resized) is in the workspace ws: luma,
// S_f, coarse search, the 8 best of it, their full-resolution SADs and the answer into res
int enqueue_batch(ssw_ctx* ctx, const std::vector<Item>& items, const Group& g, size_t b0, unsigned m, const void* const* dev_suspects,
                  uint8_t* ws, const Original& og, uint64_t* keys, uint64_t* sums, uint64_t* res, bool luma_planes) {
    hipStream_t st = ctx->stream;
    LumaBatch lb{};
    BoxBatch bb{};
    CoarseBatch cb{};
    TopBatch tb{};
    FineBatch fb{};
    unsigned nl = 0, nbox = 0, tiles = 0, max_words = 1, max_rows = 1, max_q = 1, max_qrows = 1, max_ph = 1;
    uint32_t max_n = 1;
    double bd = 0.0;
    for (unsigned s = 0; s < m; ++s) {
        const Item& it = items[b0 + s];
        uint8_t* wsi = ws + g.base_off[b0 + s - g.g0];
        const bool rs = resized(it.p), own = !g.shared[b0 + s - g.g0], f4 = it.f == 4;
        const uint8_t* lr = luma_planes ? (const uint8_t*)dev_suspects[b0 + s] : wsi + it.off_lr;
        if (own && !luma_planes) lb.it[nl++] = LumaDev{rs ? wsi + it.off_rgb : (const uint8_t*)dev_suspects[b0 + s], wsi + it.off_lr, it.p.pw, it.p.ph,
                                       rs ? 3u : it.p.channels, it.rpitch};
        max_words = std::max(max_words, it.rpitch / 4);
        max_rows = std::max(max_rows, it.p.ph);
        if (f4 && own) {
            bb.it[nbox++] = BoxDev{lr, wsi + it.off_sf, it.rpitch, it.p.pw, it.p.ph, it.tpitch, it.tw, it.th, 1u, 0u};
            max_q = std::max(max_q, it.tpitch);
            max_qrows = std::max(max_qrows, it.th);
        }
        cb.it[s] = coarse_desc(f4 ? og.phases : og.lo, f4 ? og.qpitch : og.opitch, f4 ? og.hq : og.h, f4 ? og.plane_stride : 0,
                               f4 ? wsi + it.off_sf : lr, it.tpitch, it.tw, it.th, (uint32_t*)(ws + g.d_off[b0 + s - g.g0]), it.nx, it.ny,
                               it.f, it.bx, it.by, &tiles);
        tb.it[s] = TopDev{cb.it[s].D, it.nx * it.ny, it.nx, it.skipx, it.skipy};
        max_n = std::max(max_n, it.nx * it.ny);
        fb.it[s] = FineDev{lr, it.rpitch, it.p.pw, it.p.ph, it.nx, it.bx, it.by};
        max_ph = std::max(max_ph, it.p.ph);
        bd += (double)it.nx * it.ny * ((double)it.tw * it.th);
    }
    if (nl) {
        locate_luma_kernel<<<dim3((max_words + 255) / 256, grid_rows(max_rows), nl), 256, 0, st>>>(lb);
        SSW_HIP_CHECK(hipGetLastError());
    }
    if (nbox) {
        locate_box_kernel<<<dim3((max_q + 255) / 256, grid_rows(max_qrows), nbox), 256, 0, st>>>(bb);
        SSW_HIP_CHECK(hipGetLastError());
    }
    {
        StageTimer tc(ctx, SSW_STAGE_LOCATE_COARSE, st);
        if (ctx->timing) ctx->stage_work[SSW_STAGE_LOCATE_COARSE] += bd;      // byte differences, not bytes
        locate_coarse_kernel<<<tiles, 256, 0, st>>>(cb, m);
        SSW_HIP_CHECK(hipGetLastError());
    }
    for (unsigned r = 0; r < LOC_TOP; ++r) {
        locate_topk_kernel<<<dim3(topk_blocks(max_n), m), 256, 0, st>>>(tb, keys + b0 * LOC_TOP, r);
        SSW_HIP_CHECK(hipGetLastError());
    }
    locate_fine_kernel<<<dim3(std::min(max_ph, 64u), LOC_TOP, m), 256, 0, st>>>(fb, og.lo, og.opitch, keys + b0 * LOC_TOP, sums + b0 * LOC_TOP);
    SSW_HIP_CHECK(hipGetLastError());
    locate_final_kernel<<<1, 64, 0, st>>>(fb, m, keys + b0 * LOC_TOP, sums + b0 * LOC_TOP, res + 2 * b0);
    SSW_HIP_CHECK(hipGetLastError());
    return SSW_OK;
}

}  // namespace

// The planes of n frames [h][w][3] of one size for a search of another file (angle.hip), enqueued on the context's stream: the
// luma planes, rows of `pitch` bytes (pitch % 4 == 0, bytes past w are 0) ...
int locate_luma_planes(ssw_ctx* ctx, const uint8_t* rgb, size_t n, size_t w, size_t h, uint8_t* out, size_t out_stride, unsigned pitch) {
    for (size_t i0 = 0; i0 < n; i0 += LOC_BATCH) {
        const unsigned m = (unsigned)std::min<size_t>(LOC_BATCH, n - i0);
        LumaBatch lb{};
        for (unsigned s = 0; s < m; ++s) lb.it[s] = LumaDev{rgb + (i0 + s) * w * h * 3, out + (i0 + s) * out_stride, (uint32_t)w, (uint32_t)h, 3u, pitch};
        locate_luma_kernel<<<dim3((pitch / 4 + 255) / 256, grid_rows(h), m), 256, 0, ctx->stream>>>(lb);
        SSW_HIP_CHECK(hipGetLastError());
    }
    return SSW_OK;
}
// ... and of such luma planes the decimated 4 x 4 box means S_f, [h / 4] rows of `opitch` bytes, w / 4 of them means, the others 0
int locate_box4_planes(ssw_ctx* ctx, const uint8_t* luma, size_t luma_stride, unsigned lpitch, size_t n, size_t w, size_t h, uint8_t* out,
                       size_t out_stride, unsigned opitch) {
    for (size_t i0 = 0; i0 < n; i0 += LOC_BATCH) {
        const unsigned m = (unsigned)std::min<size_t>(LOC_BATCH, n - i0);
        BoxBatch bb{};
        for (unsigned s = 0; s < m; ++s)
            bb.it[s] = BoxDev{luma + (i0 + s) * luma_stride, out + (i0 + s) * out_stride, lpitch, (uint32_t)w, (uint32_t)h, opitch, (uint32_t)(w / 4),
                              (uint32_t)(h / 4), 1u, 0u};
        locate_box_kernel<<<dim3((opitch + 255) / 256, grid_rows(h / 4), m), 256, 0, ctx->stream>>>(bb);
        SSW_HIP_CHECK(hipGetLastError());
    }
    return SSW_OK;
}

int locate_impl(ssw_ctx* ctx, const uint8_t* dev_base, size_t w, size_t h, const void* const* dev_suspects,
                const std::vector<ssw_placement>& pl, uint64_t* host_res, const std::vector<LocWindow>* win, bool luma_planes) {
    const size_t n = pl.size();
    hipStream_t st = ctx->stream;
    std::vector<Item> items;
    SSW_TRY(plan_items(pl, win, w, h, luma_planes, &items));
    const bool any_f4 = std::any_of(items.begin(), items.end(), [](const Item& it) { return it.f == 4; });
    // the original: luma plane once per call, and its 16 phase planes when a suspect takes the coarse factor 4
    const unsigned wq = (unsigned)(w / 4), hq = (unsigned)(h / 4), qpitch = (unsigned)up(std::max(wq, 1u), 4);
    const size_t plane_stride = (size_t)qpitch * hq;
    if (any_f4) SSW_TRY(grow(ctx->locate.phases, 16 * plane_stride + 16));
    uint8_t* phases = ctx->locate.phases.as<uint8_t>();
    uint64_t* keys = nullptr;
    SSW_TRY(grow_as(ctx->locate.keys, n * (2 * LOC_TOP + 2) * sizeof(uint64_t), keys));
    uint64_t* sums = keys + n * LOC_TOP;
    uint64_t* res = sums + n * LOC_TOP;
    uint8_t* lo = nullptr;
    unsigned opitch = 0;
    {
        StageTimer t(ctx, SSW_STAGE_LOCATE, st, (double)w * h * (4.0 + (any_f4 ? 2.0 : 0.0)));
        SSW_TRY(original_luma(ctx, dev_base, w, h, &lo, &opitch));
        if (any_f4) {
            BoxBatch bb{};
            bb.it[0] = BoxDev{lo, phases, opitch, (uint32_t)w, (uint32_t)h, qpitch, wq, hq, 16u, (uint32_t)plane_stride};
            locate_box_kernel<<<dim3((qpitch + 255) / 256, grid_rows(hq), 1), 256, 0, st>>>(bb);
            SSW_HIP_CHECK(hipGetLastError());
        }
        SSW_HIP_CHECK(hipMemsetAsync(keys, 0xFF, n * LOC_TOP * sizeof(uint64_t), st));
        SSW_HIP_CHECK(hipMemsetAsync(sums, 0, n * LOC_TOP * sizeof(uint64_t), st));
    }
    const Original og{lo, opitch, (unsigned)h, phases, qpitch, hq, plane_stride};
    for (size_t g0 = 0; g0 < n;) {
        const Group g = layout_group(items, g0);
        uint8_t* ws = nullptr;
        SSW_TRY(grow_as(ctx->locate.group, g.bytes + 16, ws));
        // R: the suspect resized to the size it had in the original (alpha dropped first); timed as SSW_STAGE_RESIZE
        for (size_t i = g0; i < g.g1; ++i) {
            const Item& it = items[i];
            if (!resized(it.p) || g.shared[i - g0]) continue;
            uint8_t* wsi = ws + g.base_off[i - g0];
            const uint8_t* src = (const uint8_t*)dev_suspects[i];
            if (it.p.channels == 4) {
                const size_t npix = (size_t)it.p.w * it.p.h;
                locate_strip_alpha_kernel<<<(unsigned)((npix + 255) / 256), 256, 0, st>>>(src, npix, wsi + it.off_strip);
                SSW_HIP_CHECK(hipGetLastError());
                untimed_work(ctx);
                src = wsi + it.off_strip;
            }
            const RestoreJob job{src, wsi + it.off_rgb, ssw_placement{it.p.w, it.p.h, 3u, 0u, 0u, it.p.pw, it.p.ph}};
            SSW_TRY(restore_enqueue(ctx, nullptr, it.p.pw, it.p.ph, &job, 1));
        }
        double px_bytes = 0.0;
        for (size_t i = g0; i < g.g1; ++i) {
            const Item& it = items[i];
            const double a = (double)it.p.pw * it.p.ph;
            px_bytes += a * (resized(it.p) ? 3 : it.p.channels) + a + 8.0 * it.nx * it.ny;
        }
        StageTimer t(ctx, SSW_STAGE_LOCATE, st, px_bytes);
        for (size_t b0 = g0; b0 < g.g1; b0 += LOC_BATCH)
            SSW_TRY(enqueue_batch(ctx, items, g, b0, (unsigned)std::min<size_t>(LOC_BATCH, g.g1 - b0), dev_suspects, ws, og, keys, sums, res, luma_planes));
        g0 = g.g1;
    }
    SSW_HIP_CHECK(hipMemcpyAsync(host_res, res, n * 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    untimed_work(ctx);
    SSW_HIP_CHECK(hipStreamSynchronize(st));
    return SSW_OK;
}

// ---- the scale ladder: host side ------------------------------------------------------------------------------------------------
namespace {

constexpr unsigned LAD_STEP = 8, LAD_KEEP = 8, LAD_NEAR_W = 7, LAD_NEAR_XY = 8, LAD_MIN = 32;

uint32_t ladder_height(uint64_t pw, uint64_t sw, uint64_t sh) { return (uint32_t)std::max<uint64_t>(1, (2 * sh * pw + sw) / (2 * sw)); }

struct Rung {
    uint32_t sus, pw, ph, tw, th, nx, ny;      // nx, ny: candidate positions (multiples of 4)
    RungDev dev;                               // src, T, taps and tile_begin are filled in per launch
    TapRef vt, ht;
    uint32_t tiles, channels;
    size_t lds, bytes_t, bytes_d;
};

// the rung pw x ph of a suspect p (w, h, channels); SSW_ERR_UNSUPPORTED: no LDS tile holds whole boxes of this resize
int make_rung(LadderTaps& taps, const ssw_placement& p, uint32_t sus, uint32_t pw, uint32_t ph, size_t W, size_t H, Rung* out) {
    Rung r{};
    r.sus = sus; r.pw = pw; r.ph = ph; r.tw = pw / 8; r.th = ph / 8; r.channels = p.channels;
    r.nx = (uint32_t)((W - pw) / 4 + 1); r.ny = (uint32_t)((H - ph) / 4 + 1);
    r.vt = taps.get(p.h, ph); r.ht = taps.get(p.w, pw);
    if (taps.words.size() > 0xFFFFFFFFull) return SSW_ERR_UNSUPPORTED;
    RungDev& d = r.dev;
    if (!pick_resize_tile(r.vt.shape, r.ht.shape, 8 * r.tw, 8 * r.th, p.channels, &d.tl, &r.lds, 3, 3)) return SSW_ERR_UNSUPPORTED;
    d.sw = p.w; d.ow = 8 * r.tw; d.oh = 8 * r.th; d.tpitch = (uint32_t)up(r.tw, 4);
    r.tiles = d.tl.tiles_x * d.tl.tiles_y;
    r.bytes_t = up((size_t)d.tpitch * r.th, 256);
    r.bytes_d = up((size_t)r.nx * r.ny * 4, 256);
    *out = r;
    return SSW_OK;
}

// the rung launches of rungs [b0, b1) (at most LOC_BATCH): one per channel count that occurs; T of rung i at t_ptr[i - b0]
int enqueue_rungs(ssw_ctx* ctx, const std::vector<Rung>& rungs, size_t b0, size_t b1, const void* const* dev_suspects, uint8_t* const* t_ptr,
                  const uint32_t* dev_taps) {
    static std::atomic<bool> lds_raised[64];
    SSW_TRY(resize_raise_lds_limit({reinterpret_cast<const void*>(locate_rung_kernel<3>), reinterpret_cast<const void*>(locate_rung_kernel<4>)}, lds_raised));
    double bytes = 0.0;
    for (size_t i = b0; i < b1; ++i) bytes += (double)rungs[i].dev.sw * rungs[i].channels * rungs[i].dev.oh + (double)rungs[i].tw * rungs[i].th;
    StageTimer t(ctx, SSW_STAGE_RESIZE, ctx->stream, bytes);
    for (unsigned c = 3; c <= 4; ++c) {
        RungBatch rb{};
        unsigned m = 0, tiles = 0;
        size_t lds = 0;
        for (size_t i = b0; i < b1; ++i) {
            if (rungs[i].channels != c) continue;
            RungDev& d = rb.it[m++];
            d = rungs[i].dev;
            d.src = (const uint8_t*)dev_suspects[rungs[i].sus];
            d.T = t_ptr[i - b0];
            d.taps = resize_tap_ptrs(dev_taps, rungs[i].vt, rungs[i].ht);
            d.tile_begin = tiles;
            tiles += rungs[i].tiles;
            lds = std::max(lds, rungs[i].lds);
        }
        if (!m) continue;
        if (c == 4) locate_rung_kernel<4><<<tiles, 256, lds, ctx->stream>>>(rb, m);
        else        locate_rung_kernel<3><<<tiles, 256, lds, ctx->stream>>>(rb, m);
        SSW_HIP_CHECK(hipGetLastError());
    }
    return SSW_OK;
}

}  // namespace

// (the host buffer `taps` must stay alive until the stream was waited for)
int upload_taps(ssw_ctx* ctx, const LadderTaps& taps, const uint32_t** dev) {
    SSW_TRY(grow(ctx->locate.taps, taps.words.size() * sizeof(uint32_t)));
    SSW_HIP_CHECK(hipMemcpyAsync(ctx->locate.taps.p, taps.words.data(), taps.words.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    untimed_work(ctx);
    *dev = ctx->locate.taps.as<const uint32_t>();
    return SSW_OK;
}

// pl: w, h, channels of each suspect (checked); ranges [n][2].  Waits for the stream twice: for the ladder's per-rung minima
// (the 8 kept rungs decide which widths are resized next, and restore_enqueue's launches are shaped on the host), and for the answer.
int locate_scaled_impl(ssw_ctx* ctx, const uint8_t* dev_base, size_t w, size_t h, const void* const* dev_suspects,
                       const std::vector<ssw_placement>& pl, const uint32_t* ranges, ScaledAnswer* out) {
    const size_t n = pl.size();
    hipStream_t st = ctx->stream;
    LadderTaps taps;
    std::vector<Rung> rungs;
    std::vector<size_t> first(n + 1, 0);
    for (size_t i = 0; i < n; ++i) {
        const uint32_t wmin = ranges[2 * i], wmax = ranges[2 * i + 1];
        if (wmin > wmax || std::min(wmin, ladder_height(wmin, pl[i].w, pl[i].h)) < LAD_MIN) return SSW_ERR_BAD_ARG;
        for (uint64_t pw = wmin;; pw = std::min<uint64_t>(pw + LAD_STEP, wmax)) {
            const uint32_t ph = ladder_height(pw, pl[i].w, pl[i].h);
            if (pw > w || ph > h) break;                                // both grow with the rung: every later one leaves the frame too
            Rung r;
            SSW_TRY(make_rung(taps, pl[i], (uint32_t)i, (uint32_t)pw, ph, w, h, &r));
            rungs.push_back(r);
            if (pw == wmax) break;
        }
        first[i + 1] = rungs.size();
        if (first[i + 1] == first[i]) return SSW_ERR_BAD_ARG;          // no rung fits the frame
    }
    const size_t nr = rungs.size();
    // launches of at most LOC_BATCH rungs and GROUP_BYTES of workspace (T and D of each)
    std::vector<size_t> cuts{0};
    size_t ws_bytes = 0;
    for (size_t b0 = 0; b0 < nr;) {
        size_t b1 = b0, bytes = 0;
        while (b1 < nr && b1 - b0 < LOC_BATCH && (b1 == b0 || bytes + rungs[b1].bytes_t + rungs[b1].bytes_d <= GROUP_BYTES)) {
            bytes += rungs[b1].bytes_t + rungs[b1].bytes_d;
            ++b1;
        }
        ws_bytes = std::max(ws_bytes, bytes);
        cuts.push_back(b0 = b1);
    }
    const unsigned nbx = (unsigned)((w - 8) / 4 + 1), nby = (unsigned)((h - 8) / 4 + 1);      // w, h >= 32: a rung fits
    const unsigned qpitch = (unsigned)up((nbx + 1) / 2, 4), qrows = (nby + 1) / 2;
    const size_t plane_stride = (size_t)qpitch * qrows;
    if (4 * plane_stride > 0xFFFFFFFFull) return SSW_ERR_UNSUPPORTED;
    SSW_TRY(grow(ctx->locate.box_planes, 4 * plane_stride + 16));
    SSW_TRY(grow(ctx->locate.keys, nr * LOC_TOP * sizeof(uint64_t)));
    SSW_TRY(grow(ctx->locate.group, ws_bytes + 16));
    uint8_t* planes = ctx->locate.box_planes.as<uint8_t>();
    uint64_t* keys = ctx->locate.keys.as<uint64_t>();
    uint8_t* ws = ctx->locate.group.as<uint8_t>();
    const uint32_t* dev_taps = nullptr;
    SSW_TRY(upload_taps(ctx, taps, &dev_taps));
    {
        StageTimer t(ctx, SSW_STAGE_LOCATE, st, (double)w * h * 4.5);
        uint8_t* lo = nullptr;
        unsigned opitch = 0;
        SSW_TRY(original_luma(ctx, dev_base, w, h, &lo, &opitch));
        locate_box8_kernel<<<dim3((qpitch + 255) / 256, grid_rows(qrows)), 256, 0, st>>>(lo, opitch, (unsigned)w, (unsigned)h, planes, qpitch, qrows, (unsigned)plane_stride);
        SSW_HIP_CHECK(hipGetLastError());
        SSW_HIP_CHECK(hipMemsetAsync(keys, 0xFF, nr * LOC_TOP * sizeof(uint64_t), st));
    }
    for (size_t b = 0; b + 1 < cuts.size(); ++b) {
        const size_t b0 = cuts[b], b1 = cuts[b + 1];
        const unsigned m = (unsigned)(b1 - b0);
        uint8_t* t_ptr[LOC_BATCH];
        CoarseBatch cb{};
        TopBatch tb{};
        unsigned tiles = 0;
        uint32_t max_n = 1;
        double bd = 0.0, px_bytes = 0.0;
        size_t o = 0;
        for (unsigned s = 0; s < m; ++s) {
            const Rung& r = rungs[b0 + s];
            t_ptr[s] = ws + o;
            cb.it[s] = coarse_desc(planes, qpitch, qrows, plane_stride, t_ptr[s], r.dev.tpitch, r.tw, r.th, (uint32_t*)(ws + o + r.bytes_t), r.nx, r.ny,
                                   2u, 0u, 0u, &tiles);
            tb.it[s] = TopDev{cb.it[s].D, r.nx * r.ny, 0u, 0u, 0u};
            max_n = std::max(max_n, r.nx * r.ny);
            bd += (double)r.nx * r.ny * ((double)r.tw * r.th);
            px_bytes += 8.0 * r.nx * r.ny + (double)r.tw * r.th;
            o += r.bytes_t + r.bytes_d;
        }
        SSW_TRY(enqueue_rungs(ctx, rungs, b0, b1, dev_suspects, t_ptr, dev_taps));
        StageTimer t(ctx, SSW_STAGE_LOCATE, st, px_bytes);
        {
            StageTimer tc(ctx, SSW_STAGE_LOCATE_COARSE, st);
            if (ctx->timing) ctx->stage_work[SSW_STAGE_LOCATE_COARSE] += bd;          // byte differences, not bytes
            locate_coarse_kernel<<<tiles, 256, 0, st>>>(cb, m);
            SSW_HIP_CHECK(hipGetLastError());
        }
        // the rung's smallest (D, y, x): round 0 of the top-k, an atomic minimum of the 64-bit key
        locate_topk_kernel<<<dim3(topk_blocks(max_n), m), 256, 0, st>>>(tb, keys + b0 * LOC_TOP, 0);
        SSW_HIP_CHECK(hipGetLastError());
    }
    std::vector<uint64_t> hk(nr * LOC_TOP);
    SSW_HIP_CHECK(hipMemcpyAsync(hk.data(), keys, hk.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    untimed_work(ctx);
    SSW_HIP_CHECK(hipStreamSynchronize(st));
    // on the host: the 8 rungs with the smallest D / n, then the windowed searches around them
    std::vector<ssw_placement> rp;
    std::vector<LocWindow> win;
    std::vector<const void*> rsus;
    std::vector<size_t> owner;
    for (size_t i = 0; i < n; ++i) {
        const uint32_t wmin = ranges[2 * i], wmax = ranges[2 * i + 1];
        std::vector<size_t> order;
        for (size_t j = first[i]; j < first[i + 1]; ++j) order.push_back(j);
        auto D = [&](size_t j) { return hk[j * LOC_TOP] >> 32; };
        auto N = [&](size_t j) { return (uint64_t)rungs[j].tw * rungs[j].th; };
        std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return D(a) * N(b) < D(b) * N(a); });
        if (order.size() > LAD_KEEP) order.resize(LAD_KEEP);
        struct Job { uint32_t pw, ph; LocWindow w; };
        std::vector<Job> jobs;
        for (size_t j : order) {
            const Rung& r = rungs[j];
            const uint32_t idx = (uint32_t)hk[j * LOC_TOP];
            const int64_t xj = 4 * (int64_t)(idx % r.nx), yj = 4 * (int64_t)(idx / r.nx);
            for (int64_t pw = std::max<int64_t>(wmin, (int64_t)r.pw - LAD_NEAR_W); pw <= std::min<int64_t>(wmax, (int64_t)r.pw + LAD_NEAR_W); ++pw) {
                const uint32_t ph = ladder_height((uint64_t)pw, pl[i].w, pl[i].h);
                if ((uint64_t)pw > w || ph > h) continue;
                const int64_t x0 = std::max<int64_t>(0, xj - LAD_NEAR_XY), x1 = std::min<int64_t>((int64_t)w - pw, xj + LAD_NEAR_XY);
                const int64_t y0 = std::max<int64_t>(0, yj - LAD_NEAR_XY), y1 = std::min<int64_t>((int64_t)h - ph, yj + LAD_NEAR_XY);
                if (x0 > x1 || y0 > y1) continue;
                const Job job{(uint32_t)pw, ph, LocWindow{(uint32_t)x0, (uint32_t)x1, (uint32_t)y0, (uint32_t)y1, false}};
                bool seen = false;
                for (const Job& q : jobs) seen |= q.pw == job.pw && q.w.x0 == job.w.x0 && q.w.x1 == job.w.x1 && q.w.y0 == job.w.y0 && q.w.y1 == job.w.y1;
                if (!seen) jobs.push_back(job);
            }
        }
        std::stable_sort(jobs.begin(), jobs.end(), [](const Job& a, const Job& b) { return a.pw < b.pw; });       // a width's searches side by side: one resize
        for (size_t q = 0; q < jobs.size(); ++q) {
            ssw_placement p = pl[i];
            p.x = p.y = 0; p.pw = jobs[q].pw; p.ph = jobs[q].ph;
            LocWindow lw = jobs[q].w;
            lw.share = q > 0 && jobs[q - 1].pw == jobs[q].pw;
            rp.push_back(p); win.push_back(lw); rsus.push_back(dev_suspects[i]); owner.push_back(i);
        }
    }
    SSW_TRY(restore_prepare_rgb(ctx, rp));
    std::vector<uint64_t> res(2 * rp.size());
    SSW_TRY(locate_impl(ctx, dev_base, w, h, rsus.data(), rp, res.data(), &win));
    std::vector<char> have(n, 0);
    for (size_t q = 0; q < rp.size(); ++q) {
        ScaledAnswer a{rp[q].pw, rp[q].ph, (uint32_t)res[2 * q + 1], (uint32_t)(res[2 * q + 1] >> 32), res[2 * q]};
        ScaledAnswer& b = out[owner[q]];
        bool better = !have[owner[q]];
        if (!better) {                                                  // smallest SAD / (pw ph), then pw, y, x; 255 * 2^26 * 2^26 fits 64 bits
            const uint64_t l = a.sad * ((uint64_t)b.pw * b.ph), r = b.sad * ((uint64_t)a.pw * a.ph);
            better = l != r ? l < r : a.pw != b.pw ? a.pw < b.pw : a.y != b.y ? a.y < b.y : a.x < b.x;
        }
        if (better) { b = a; have[owner[q]] = 1; }
    }
    return SSW_OK;
}

// T_j of one rung alone (ssw_locate_rung_boxes): what locate_rung_kernel stores, compact on the host
int rung_boxes_impl(ssw_ctx* ctx, const void* dev_suspect, const ssw_placement& p, uint8_t* host_t) {
    LadderTaps taps;
    std::vector<Rung> rungs(1);
    SSW_TRY(make_rung(taps, p, 0u, p.pw, p.ph, p.pw, p.ph, &rungs[0]));
    const Rung& r = rungs[0];
    SSW_TRY(grow(ctx->locate.group, r.bytes_t + 16));
    uint8_t* t_ptr[1] = {ctx->locate.group.as<uint8_t>()};
    const uint32_t* dev_taps = nullptr;
    SSW_TRY(upload_taps(ctx, taps, &dev_taps));
    SSW_TRY(enqueue_rungs(ctx, rungs, 0, 1, &dev_suspect, t_ptr, dev_taps));
    std::vector<uint8_t> t((size_t)r.dev.tpitch * r.th);
    SSW_HIP_CHECK(hipMemcpyAsync(t.data(), t_ptr[0], t.size(), hipMemcpyDeviceToHost, ctx->stream));
    untimed_work(ctx);
    SSW_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    for (uint32_t k = 0; k < r.th; ++k) std::memcpy(host_t + (size_t)k * r.tw, t.data() + (size_t)k * r.dev.tpitch, r.tw);
    return SSW_OK;
}

// ---- for the ladder of another file (locate_turned.hip) ------------------------------------------------------------------------
static_assert(LOCATE_KEY_STRIDE == LOC_TOP && LOCATE_BATCH == LOC_BATCH, "ssw_host.hpp states both");

int locate_box8_planes(ssw_ctx* ctx, const uint8_t* dev_base, size_t w, size_t h, const uint8_t** planes, unsigned* qpitch, unsigned* qrows,
                       size_t* plane_stride) {
    const unsigned nbx = (unsigned)((w - 8) / 4 + 1), nby = (unsigned)((h - 8) / 4 + 1);
    *qpitch = (unsigned)up((nbx + 1) / 2, 4); *qrows = (nby + 1) / 2;
    *plane_stride = (size_t)*qpitch * *qrows;
    if (4 * *plane_stride > 0xFFFFFFFFull) return SSW_ERR_UNSUPPORTED;
    uint8_t* out = nullptr;
    SSW_TRY(grow_as(ctx->locate.box_planes, 4 * *plane_stride + 16, out));
    StageTimer t(ctx, SSW_STAGE_LOCATE, ctx->stream, (double)w * h * 4.5);
    uint8_t* lo = nullptr;
    unsigned opitch = 0;
    SSW_TRY(original_luma(ctx, dev_base, w, h, &lo, &opitch));
    locate_box8_kernel<<<dim3((*qpitch + 255) / 256, grid_rows(*qrows)), 256, 0, ctx->stream>>>(lo, opitch, (unsigned)w, (unsigned)h, out, *qpitch, *qrows,
                                                                                                   (unsigned)*plane_stride);
    SSW_HIP_CHECK(hipGetLastError());
    *planes = out;
    return SSW_OK;
}

int locate_box_searches(ssw_ctx* ctx, const uint8_t* planes, unsigned qpitch, unsigned qrows, size_t plane_stride, const BoxSearch* it, unsigned m,
                        uint64_t* keys) {
    CoarseBatch cb{};
    TopBatch tb{};
    unsigned tiles = 0;
    uint32_t max_n = 1;
    double bd = 0.0, px_bytes = 0.0;
    for (unsigned s = 0; s < m; ++s) {
        const BoxSearch& b = it[s];
        cb.it[s] = coarse_desc(planes, qpitch, qrows, plane_stride, b.T, b.tpitch, b.tw, b.th, b.D, b.nx, b.ny, 2u, 0u, 0u, &tiles);
        tb.it[s] = TopDev{b.D, b.nx * b.ny, 0u, 0u, 0u};
        max_n = std::max(max_n, b.nx * b.ny);
        bd += (double)b.nx * b.ny * ((double)b.tw * b.th);
        px_bytes += 8.0 * b.nx * b.ny + (double)b.tw * b.th;
    }
    StageTimer t(ctx, SSW_STAGE_LOCATE, ctx->stream, px_bytes);
    {
        StageTimer tc(ctx, SSW_STAGE_LOCATE_COARSE, ctx->stream);
        if (ctx->timing) ctx->stage_work[SSW_STAGE_LOCATE_COARSE] += bd;              // byte differences, not bytes
        locate_coarse_kernel<<<tiles, 256, 0, ctx->stream>>>(cb, m);
        SSW_HIP_CHECK(hipGetLastError());
    }
    locate_topk_kernel<<<dim3(topk_blocks(max_n), m), 256, 0, ctx->stream>>>(tb, keys, 0);
    SSW_HIP_CHECK(hipGetLastError());
    return SSW_OK;
}

}  // namespace host
}  // namespace ssw

extern "C" int ssw_locate_rgb8(ssw_ctx* ctx, const uint8_t* dev_base_rgb, size_t w, size_t h, const void* const* dev_suspects,
                               ssw_placement* placements, size_t n, uint64_t* host_sad) {
    using namespace ssw::host;
    if (!ctx) return SSW_ERR_BAD_ARG;
    if (n == 0) return SSW_OK;
    if (!dev_base_rgb || !dev_suspects || !placements || !host_sad) return SSW_ERR_BAD_ARG;
    std::vector<ssw_placement> in(placements, placements + n), pl;
    for (ssw_placement& p : in) p.x = p.y = 0;                     // outputs: what the caller left there is not read
    SSW_TRY(restore_normalise(in.data(), n, w, h, &pl));
    for (size_t i = 0; i < n; ++i) if (!dev_suspects[i]) return SSW_ERR_BAD_ARG;
    CtxGuard g(ctx);
    SSW_TRY(restore_prepare_rgb(ctx, pl));
    std::vector<uint64_t> res(2 * n);
    SSW_TRY(locate_impl(ctx, dev_base_rgb, w, h, dev_suspects, pl, res.data()));
    for (size_t i = 0; i < n; ++i) {
        host_sad[i] = res[2 * i];
        placements[i].x = (uint32_t)res[2 * i + 1];
        placements[i].y = (uint32_t)(res[2 * i + 1] >> 32);
    }
    return SSW_OK;
}

extern "C" int ssw_locate_scaled_rgb8(ssw_ctx* ctx, const uint8_t* dev_base_rgb, size_t w, size_t h, const void* const* dev_suspects,
                                      ssw_placement* placements, const ssw_scale_range* ranges, size_t n, uint64_t* host_sad) {
    using namespace ssw::host;
    if (!ctx) return SSW_ERR_BAD_ARG;
    if (n == 0) return SSW_OK;
    if (!dev_base_rgb || !dev_suspects || !placements || !ranges || !host_sad) return SSW_ERR_BAD_ARG;
    std::vector<ssw_placement> in(placements, placements + n), pl;
    for (ssw_placement& p : in) p.x = p.y = p.pw = p.ph = 0;          // outputs: what the caller left there is not read
    if (w == 0 || h == 0 || w > 0xFFFFFFFFull || h > 0xFFFFFFFFull) return SSW_ERR_BAD_ARG;
    for (const ssw_placement& p : in)
        if ((p.channels != 3 && p.channels != 4) || p.w == 0 || p.h == 0 || (uint64_t)p.w * p.channels > 0xFFFFFFFFull) return SSW_ERR_BAD_ARG;
    for (size_t i = 0; i < n; ++i) if (!dev_suspects[i]) return SSW_ERR_BAD_ARG;
    CtxGuard g(ctx);
    std::vector<ScaledAnswer> ans(n);
    std::vector<uint32_t> r(2 * n);
    for (size_t i = 0; i < n; ++i) { r[2 * i] = ranges[i].wmin; r[2 * i + 1] = ranges[i].wmax; }
    SSW_TRY(locate_scaled_impl(ctx, dev_base_rgb, w, h, dev_suspects, in, r.data(), ans.data()));
    for (size_t i = 0; i < n; ++i) {
        placements[i].pw = ans[i].pw; placements[i].ph = ans[i].ph;
        placements[i].x = ans[i].x; placements[i].y = ans[i].y;
        host_sad[i] = ans[i].sad;
    }
    return SSW_OK;
}

extern "C" int ssw_locate_rung_boxes(ssw_ctx* ctx, const void* dev_suspect, size_t sw, size_t sh, size_t channels, size_t pw, size_t ph,
                                     uint8_t* host_boxes) {
    using namespace ssw::host;
    if (!ctx || !dev_suspect || !host_boxes) return SSW_ERR_BAD_ARG;
    if ((channels != 3 && channels != 4) || sw == 0 || sh == 0 || pw < 8 || ph < 8 || sw * channels > 0xFFFFFFFFull || sh > 0xFFFFFFFFull ||
        pw > 0xFFFFFFFFull || ph > 0xFFFFFFFFull) return SSW_ERR_BAD_ARG;
    CtxGuard g(ctx);
    return rung_boxes_impl(ctx, dev_suspect, ssw_placement{(uint32_t)sw, (uint32_t)sh, (uint32_t)channels, 0u, 0u, (uint32_t)pw, (uint32_t)ph}, host_boxes);
}
