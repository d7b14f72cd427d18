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
#include <algorithm>
#include <vector>

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
    uint32_t nx, ny, f;
    uint32_t tiles_x, tiles_y, tile_begin;
};
struct CoarseBatch { CoarseDev it[LOC_BATCH]; };
struct TopDev { const uint32_t* D; uint32_t n; };
struct TopBatch { TopDev it[LOC_BATCH]; };
struct FineDev { const uint8_t* lr; uint32_t rpitch, pw, ph, nx; };
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
    const unsigned px = d.f == 4 ? (phase & 3) : 0, py = d.f == 4 ? (phase >> 2) : 0;
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
                const unsigned row = y0 + j0 + r, wd = (x0 + i0) / 4 + c;
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
    const uint32_t idx = (uint32_t)key, y = idx / d.nx, x = idx - y * d.nx;
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
    const uint32_t y = best_idx / b.it[s].nx, x = best_idx - y * b.it[s].nx;
    res[2 * s] = best;
    res[2 * s + 1] = ((uint64_t)y << 32) | x;
}

namespace host {

namespace {

size_t up(size_t v, size_t a) { return (v + a - 1) / a * a; }
unsigned grid_rows(size_t rows) { return (unsigned)std::min<size_t>(std::max<size_t>(rows, 1), 65535); }

// what one suspect needs of the group's workspace, as offsets into it
struct Item {
    size_t index;                 // position in the call
    ssw_placement p;              // normalised, x = y = 0
    unsigned f, nx, ny;           // coarse factor, candidate positions
    unsigned rpitch, tw, th, tpitch;
    size_t off_rgb, off_strip, off_lr, off_sf, off_d, bytes;
};

constexpr size_t GROUP_BYTES = 256u << 20;      // workspace of one group of suspects (one suspect may need more)

}  // namespace

int locate_impl(ssw_ctx* ctx, const uint8_t* dev_base, size_t w, size_t h, const void* const* dev_suspects,
                const std::vector<ssw_placement>& pl, uint64_t* host_res) {
    const size_t n = pl.size();
    hipStream_t st = ctx->stream;
    std::vector<Item> items(n);
    bool any_f4 = false;
    for (size_t i = 0; i < n; ++i) {
        Item& it = items[i];
        it.index = i;
        it.p = pl[i];
        it.f = std::min(it.p.pw, it.p.ph) >= 64 ? 4u : 1u;
        any_f4 |= it.f == 4;
        it.nx = (unsigned)(w - it.p.pw + 1);
        it.ny = (unsigned)(h - it.p.ph + 1);
        if ((uint64_t)it.nx * it.ny > 0xFFFFFFFFull) return SSW_ERR_UNSUPPORTED;      // a position is 32 bits of the key
        it.rpitch = (unsigned)up(it.p.pw, 4);
        it.tw = it.f == 4 ? it.p.pw / 4 : it.p.pw;
        it.th = it.f == 4 ? it.p.ph / 4 : it.p.ph;
        it.tpitch = it.f == 4 ? (unsigned)up(it.tw, 4) : it.rpitch;
        const bool rs = it.p.pw != it.p.w || it.p.ph != it.p.h;
        size_t o = 0;
        it.off_rgb = o;   o += rs ? up((size_t)it.p.pw * it.p.ph * 3, 256) : 0;
        it.off_strip = o; o += rs && it.p.channels == 4 ? up((size_t)it.p.w * it.p.h * 3, 256) : 0;
        it.off_lr = o;    o += up((size_t)it.rpitch * it.p.ph, 256);
        it.off_sf = o;    o += it.f == 4 ? up((size_t)it.tpitch * it.th, 256) : 0;
        it.off_d = o;     o += up((size_t)it.nx * it.ny * 4, 256);
        it.bytes = o;
    }
    // the original: luma plane once per call, and its 16 phase planes when a suspect takes the coarse factor 4
    const unsigned opitch = (unsigned)up(w, 4);
    const unsigned wq = (unsigned)(w / 4), hq = (unsigned)(h / 4), qpitch = (unsigned)up(std::max(wq, 1u), 4);
    const size_t plane_stride = (size_t)qpitch * hq;
    SSW_TRY(grow(ctx->locate[0], (size_t)opitch * h + 16));
    if (any_f4) SSW_TRY(grow(ctx->locate[1], 16 * plane_stride + 16));
    SSW_TRY(grow(ctx->locate[3], n * (2 * LOC_TOP + 2) * sizeof(uint64_t)));
    uint8_t* lo = (uint8_t*)ctx->locate[0].p;
    uint8_t* phases = (uint8_t*)ctx->locate[1].p;
    uint64_t* keys = (uint64_t*)ctx->locate[3].p;
    uint64_t* sums = keys + n * LOC_TOP;
    uint64_t* res = sums + n * LOC_TOP;
    {
        StageTimer t(ctx, SSW_STAGE_LOCATE, st, (double)w * h * (4.0 + (any_f4 ? 2.0 : 0.0)));
        SSW_HIP_CHECK(hipMemsetAsync(lo + (size_t)opitch * h, 0, 16, st));
        LumaBatch lb{};
        lb.it[0] = LumaDev{dev_base, lo, (uint32_t)w, (uint32_t)h, 3u, opitch};
        locate_luma_kernel<<<dim3((opitch / 4 + 255) / 256, grid_rows(h), 1), 256, 0, st>>>(lb);
        SSW_HIP_CHECK(hipGetLastError());
        if (any_f4) {
            BoxBatch bb{};
            bb.it[0] = BoxDev{lo, phases, opitch, (uint32_t)w, (uint32_t)h, qpitch, wq, hq, 16u, (uint32_t)plane_stride};
            locate_box_kernel<<<dim3((qpitch + 255) / 256, grid_rows(hq), 1), 256, 0, st>>>(bb);
            SSW_HIP_CHECK(hipGetLastError());
        }
        SSW_HIP_CHECK(hipMemsetAsync(keys, 0xFF, n * LOC_TOP * sizeof(uint64_t), st));
        SSW_HIP_CHECK(hipMemsetAsync(sums, 0, n * LOC_TOP * sizeof(uint64_t), st));
    }
    // suspects in groups of bounded workspace, in the order of the call
    for (size_t g0 = 0; g0 < n;) {
        size_t g1 = g0, bytes = 0;
        while (g1 < n && (g1 == g0 || bytes + items[g1].bytes <= GROUP_BYTES)) bytes += items[g1++].bytes;
        SSW_TRY(grow(ctx->locate[2], bytes + 16));
        uint8_t* ws = (uint8_t*)ctx->locate[2].p;
        std::vector<size_t> base_off(g1 - g0);
        for (size_t i = g0, o = 0; i < g1; ++i) { base_off[i - g0] = o; o += items[i].bytes; }
        // 1. R: the suspect resized to the size it had in the original (alpha dropped first); timed as SSW_STAGE_RESIZE
        for (size_t i = g0; i < g1; ++i) {
            const Item& it = items[i];
            if (it.p.pw == it.p.w && it.p.ph == it.p.h) continue;
            uint8_t* wsi = ws + base_off[i - g0];
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
        for (size_t i = g0; i < g1; ++i) {
            const Item& it = items[i];
            const double a = (double)it.p.pw * it.p.ph;
            px_bytes += a * (it.p.pw == it.p.w && it.p.ph == it.p.h ? it.p.channels : 3) + a + 8.0 * it.nx * it.ny;
        }
        StageTimer t(ctx, SSW_STAGE_LOCATE, st, px_bytes);
        for (size_t b0 = g0; b0 < g1; b0 += LOC_BATCH) {
            const unsigned m = (unsigned)std::min<size_t>(LOC_BATCH, g1 - b0);
            LumaBatch lb{};
            BoxBatch bb{};
            CoarseBatch cb{};
            TopBatch tb{};
            FineBatch fb{};
            unsigned nbox = 0, tiles = 0, max_words = 1, max_rows = 1, max_q = 1, max_qrows = 1, max_ph = 1;
            uint32_t max_n = 1;
            for (unsigned s = 0; s < m; ++s) {
                const Item& it = items[b0 + s];
                uint8_t* wsi = ws + base_off[b0 + s - g0];
                const bool rs = it.p.pw != it.p.w || it.p.ph != it.p.h;
                lb.it[s] = LumaDev{rs ? wsi + it.off_rgb : (const uint8_t*)dev_suspects[b0 + s], wsi + it.off_lr, it.p.pw, it.p.ph,
                                   rs ? 3u : it.p.channels, it.rpitch};
                max_words = std::max(max_words, it.rpitch / 4);
                max_rows = std::max(max_rows, it.p.ph);
                if (it.f == 4) {
                    bb.it[nbox++] = BoxDev{wsi + it.off_lr, wsi + it.off_sf, it.rpitch, it.p.pw, it.p.ph, it.tpitch, it.tw, it.th, 1u, 0u};
                    max_q = std::max(max_q, it.tpitch);
                    max_qrows = std::max(max_qrows, it.th);
                }
                CoarseDev& c = cb.it[s];
                c.plane = it.f == 4 ? phases : lo;
                c.tmpl = wsi + (it.f == 4 ? it.off_sf : it.off_lr);
                c.D = (uint32_t*)(wsi + it.off_d);
                c.ppitch = it.f == 4 ? qpitch : opitch;
                c.prows = it.f == 4 ? hq : (uint32_t)h;
                c.plane_stride = it.f == 4 ? (uint32_t)plane_stride : 0u;
                c.tpitch = it.tpitch; c.tw = it.tw; c.th = it.th;
                c.nx = it.nx; c.ny = it.ny; c.f = it.f;
                c.tiles_x = ((it.nx + it.f - 1) / it.f + LOC_TX - 1) / LOC_TX;
                c.tiles_y = ((it.ny + it.f - 1) / it.f + LOC_TY - 1) / LOC_TY;
                c.tile_begin = tiles;
                tiles += c.tiles_x * c.tiles_y * it.f * it.f;
                tb.it[s] = TopDev{c.D, it.nx * it.ny};
                max_n = std::max(max_n, it.nx * it.ny);
                fb.it[s] = FineDev{wsi + it.off_lr, it.rpitch, it.p.pw, it.p.ph, it.nx};
                max_ph = std::max(max_ph, it.p.ph);
            }
            locate_luma_kernel<<<dim3((max_words + 255) / 256, grid_rows(max_rows), m), 256, 0, st>>>(lb);
            SSW_HIP_CHECK(hipGetLastError());
            if (nbox) {
                locate_box_kernel<<<dim3((max_q + 255) / 256, grid_rows(max_qrows), nbox), 256, 0, st>>>(bb);
                SSW_HIP_CHECK(hipGetLastError());
            }
            {
                double bd = 0.0;
                for (unsigned s = 0; s < m; ++s) bd += (double)items[b0 + s].nx * items[b0 + s].ny * ((double)items[b0 + s].tw * items[b0 + s].th);
                StageTimer tc(ctx, SSW_STAGE_LOCATE_COARSE, st);
                if (ctx->timing) ctx->stage_work[SSW_STAGE_LOCATE_COARSE] += bd;      // byte differences, not bytes
                locate_coarse_kernel<<<tiles, 256, 0, st>>>(cb, m);
                SSW_HIP_CHECK(hipGetLastError());
            }
            const unsigned tblocks = (unsigned)std::min<size_t>(((size_t)max_n + 2047) / 2048, 512);
            for (unsigned r = 0; r < LOC_TOP; ++r) {
                locate_topk_kernel<<<dim3(tblocks, m), 256, 0, st>>>(tb, keys + b0 * LOC_TOP, r);
                SSW_HIP_CHECK(hipGetLastError());
            }
            locate_fine_kernel<<<dim3(std::min(max_ph, 64u), LOC_TOP, m), 256, 0, st>>>(fb, lo, opitch, keys + b0 * LOC_TOP, sums + b0 * LOC_TOP);
            SSW_HIP_CHECK(hipGetLastError());
            locate_final_kernel<<<1, 64, 0, st>>>(fb, m, keys + b0 * LOC_TOP, sums + b0 * LOC_TOP, res + 2 * b0);
            SSW_HIP_CHECK(hipGetLastError());
        }
        g0 = g1;
    }
    SSW_HIP_CHECK(hipMemcpyAsync(host_res, res, n * 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    untimed_work(ctx);
    SSW_HIP_CHECK(hipStreamSynchronize(st));
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
    {   // the resize runs on the colour channels alone
        std::vector<ssw_placement> rgb(pl);
        for (ssw_placement& p : rgb) p.channels = 3;
        SSW_TRY(restore_prepare(ctx, rgb));
    }
    std::vector<uint64_t> res(2 * n);
    SSW_TRY(locate_impl(ctx, dev_base_rgb, w, h, dev_suspects, pl, res.data()));
    for (size_t i = 0; i < n; ++i) {
        host_sad[i] = res[2 * i];
        placements[i].x = (uint32_t)res[2 * i + 1];
        placements[i].y = (uint32_t)(res[2 * i + 1] >> 32);
    }
    return SSW_OK;
}
