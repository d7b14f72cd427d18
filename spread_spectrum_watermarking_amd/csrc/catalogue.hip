// Identifying a suspect's original (ssw_signature_rgb8, ssw_signature_match): which of a few thousand -- or a million -- originals
// is this picture a copy of?  Every frame gets a signature of 1024 bytes, the rounded mean luma of the cells of a 32 x 32 grid,
// and a suspect's signature is compared with every signature of the catalogue by the sum of absolute byte differences.
// include/ssw.h states the definition; every quantity is an integer, so nothing here depends on the order of a sum and the
// result equals the numpy restatement of tests/test_identify_cpu.py exactly.  The reference has no counterpart: its `test`
// command (examples/main.rs:369-415) is handed the original.
//
// Kernels:
//   signature_kernel      frames of different sizes and channel counts in one launch (descriptors as kernel arguments, 32 per
//                         launch, like restore.hip's and locate.hip's).  One block owns one row of cells of one frame, or -- wide
//                         frames -- a run of cell columns of it, so that one 8K frame alone is 256 blocks; a block owns whole
//                         cells, so no sum crosses blocks and nothing is atomic in global memory.  A thread keeps its four pixel
//                         columns for all rows of the cell row (the cell of a column is found once, outside the row loop) and
//                         reads 12 / 16 bytes per row with one load; no alignment is assumed of anything.  HBM-bound: w h c
//                         bytes in, 1024 out.
//   match_kernel          THE HOT PATH, a SAD "GEMM": a tile of 16 or 128 query signatures against tiles of 128 catalogue
//                         signatures, 256 bytes of every signature at a time in LDS; a thread owns 1 or 8 queries x 8 entries and
//                         sums four bytes per v_sad_u8, sixteen-byte LDS reads, the next slab's global loads in flight beside
//                         them.  Catalogue bytes leave HBM once per query tile.  A block keeps, per query, the 8 smallest keys
//                         (D << 32) | index it has seen, sorted, in LDS: a tile's distances are compared with the 8th, and the few
//                         that pass are inserted by the wave that owns the row.  The lists live in global memory between the
//                         launches of a call (one launch per chunk of 32768 entries), one per (block, query).
//   match_finish_kernel   one wave per query: the `top` smallest keys of all blocks' lists, in order
#include <algorithm>
#include <atomic>
#include <cstring>
#include <vector>

#include "ssw_host.hpp"

namespace ssw {

constexpr unsigned SIG_GRID = 32;                 // cells per axis
constexpr unsigned SIG_BYTES = SIG_GRID * SIG_GRID;
constexpr unsigned SIG_BATCH = 32;                // frames per launch

struct SigDev { const uint8_t* src; uint32_t w, h, c, split; };      // split: 1, 2, 4 or 8 blocks per row of cells
struct SigBatch { SigDev it[SIG_BATCH]; };

__device__ inline uint32_t sig_luma(uint32_t r, uint32_t g, uint32_t b) { return (77u * r + 150u * g + 29u * b + 128u) >> 8; }

// the lumas of four whole pixels at p, one load (the compiler emits global_load_dwordx3 / x4 for a byte-aligned copy)
template <unsigned C>
__device__ inline void sig_load4(const uint8_t* __restrict__ p, uint32_t (&l)[4]) {
    if (C == 3) {
        uint32_t v[3];
        __builtin_memcpy(v, p, 12);
        l[0] = sig_luma(v[0] & 255u, (v[0] >> 8) & 255u, (v[0] >> 16) & 255u);
        l[1] = sig_luma(v[0] >> 24, v[1] & 255u, (v[1] >> 8) & 255u);
        l[2] = sig_luma((v[1] >> 16) & 255u, v[1] >> 24, v[2] & 255u);
        l[3] = sig_luma((v[2] >> 8) & 255u, (v[2] >> 16) & 255u, v[2] >> 24);
    } else {
        uint32_t v[4];
        __builtin_memcpy(v, p, 16);
#pragma unroll
        for (unsigned i = 0; i < 4; ++i) l[i] = sig_luma(v[i] & 255u, (v[i] >> 8) & 255u, (v[i] >> 16) & 255u);
    }
}

// The cells [i0, i0 + cells) of cell row j of one frame.  s_bx: the 33 column boundaries of the frame; s_cell: zero on entry.
template <unsigned C>
__device__ inline void sig_cell_row(const SigDev& d, unsigned i0, unsigned cells, unsigned y0, unsigned y1, const uint32_t* s_bx, uint32_t* s_cell) {
    const unsigned xa = s_bx[i0], xb = s_bx[i0 + cells];
    const unsigned groups = (xb - xa + 3) / 4;            // of four pixel columns
    unsigned lx = 0;
    while ((1u << lx) < groups && lx < 8) ++lx;
    const unsigned tx = threadIdx.x & ((1u << lx) - 1), ty = threadIdx.x >> lx, ny = 256u >> lx;
    for (unsigned gi = tx; gi < groups; gi += 1u << lx) {
        const unsigned x0 = xa + 4 * gi;
        // the cell of each of the four columns: one division, then at most one step per column (no cell is empty)
        unsigned ci[4];
        bool valid[4];
        ci[0] = (unsigned)((32ull * x0 + 31) / d.w);      // x0 < w: at most 31
#pragma unroll
        for (unsigned p = 0; p < 4; ++p) {
            valid[p] = x0 + p < xb;
            if (p) ci[p] = ci[p - 1] + (valid[p] && x0 + p >= s_bx[ci[p - 1] + 1] ? 1u : 0u);
        }
        const bool wide = x0 + 4 <= d.w;                  // four whole pixels of this row: never reads past the frame
        uint32_t acc[4] = {0, 0, 0, 0};
#pragma unroll 4
        for (unsigned y = y0 + ty; y < y1; y += ny) {
            const uint8_t* __restrict__ p = d.src + ((size_t)y * d.w + x0) * C;
            uint32_t l[4] = {0, 0, 0, 0};
            if (wide) sig_load4<C>(p, l);
            else
                for (unsigned q = 0; q < 4 && x0 + q < d.w; ++q) l[q] = sig_luma(p[q * C], p[q * C + 1], p[q * C + 2]);
#pragma unroll
            for (unsigned q = 0; q < 4; ++q) acc[q] += l[q];
        }
        // columns of one cell first summed in the thread, then one LDS add per cell the thread touches (integers: any order)
        uint32_t run = 0;
#pragma unroll
        for (unsigned p = 0; p < 4; ++p) {
            if (valid[p]) run += acc[p];
            const bool last = p == 3 || !valid[p + 1] || ci[p + 1] != ci[p];
            if (valid[p] && last) { if (run) atomicAdd(&s_cell[ci[p] - i0], run); run = 0; }
        }
    }
}

// grid: (32 * gsplit, frames of the launch), gsplit = the largest split of the launch.  out: [frames][1024]
__global__ __launch_bounds__(256) void signature_kernel(SigBatch b, unsigned gsplit, uint8_t* __restrict__ out) {
    __shared__ uint32_t s_bx[SIG_GRID + 1];
    __shared__ uint32_t s_cell[SIG_GRID];
    const SigDev& d = b.it[blockIdx.y];
    const unsigned j = blockIdx.x / gsplit, g = blockIdx.x % gsplit;
    if (g >= d.split) return;                             // uniform
    const unsigned cells = SIG_GRID / d.split, i0 = g * cells;
    const unsigned y0 = (unsigned)((uint64_t)j * d.h / SIG_GRID), y1 = (unsigned)((uint64_t)(j + 1) * d.h / SIG_GRID);
    if (threadIdx.x <= SIG_GRID) s_bx[threadIdx.x] = (uint32_t)((uint64_t)threadIdx.x * d.w / SIG_GRID);
    if (threadIdx.x < SIG_GRID) s_cell[threadIdx.x] = 0;
    __syncthreads();
    if (d.c == 3) sig_cell_row<3>(d, i0, cells, y0, y1, s_bx, s_cell);
    else sig_cell_row<4>(d, i0, cells, y0, y1, s_bx, s_cell);
    __syncthreads();
    if (threadIdx.x < cells) {
        const unsigned i = i0 + threadIdx.x;
        const uint32_t n = (s_bx[i + 1] - s_bx[i]) * (y1 - y0);
        out[(size_t)blockIdx.y * SIG_BYTES + j * SIG_GRID + i] = (uint8_t)((s_cell[threadIdx.x] + n / 2) / n);
    }
}

// ---- match -----------------------------------------------------------------------------------------------------------------------
constexpr unsigned MT_C = 128;                    // catalogue entries of a tile
constexpr unsigned MT_Q = 128;                    // queries of the large tile (the small one: 16)
constexpr unsigned MT_SLAB = 256;                 // bytes of every signature that are in LDS at a time
constexpr unsigned MT_PITCH = MT_SLAB + 16;       // LDS row pitch: rows r and r + 1 are one 16-byte bank group apart
constexpr unsigned MT_TOP = 8;
constexpr unsigned MATCH_CHUNK = 32768;           // catalogue entries of one launch
constexpr unsigned MATCH_GRID = 256;              // blocks of a launch = lists per query
constexpr uint64_t MT_NONE = ~0ull;
constexpr size_t MT_PART_BYTES = (size_t)MATCH_GRID * MT_Q * MT_TOP * sizeof(uint64_t);
constexpr size_t match_lds_bytes(unsigned qt) { return (size_t)(qt + MT_C) * MT_PITCH + (size_t)qt * MT_TOP * sizeof(uint64_t); }

__device__ inline uint64_t wave_min_u64(uint64_t m) {
#pragma unroll
    for (int o = 32; o; o >>= 1) { const uint64_t v = __shfl_xor(m, o); m = v < m ? v : m; }
    return m;
}

// One block: the queries [q0, q0 + 16 QPT) against the tiles blockIdx.x, blockIdx.x + gridDim.x, ... of the catalogue entries
// [c_begin, c_end).  Thread (tq, tc) = (t / 16, t % 16) owns the queries f 16 + tq and the entries e 16 + tc: within a wave the
// sixteen lanes of a b128 read group read sixteen consecutive rows (different bank groups) or the same address (broadcast).
// part: [MATCH_GRID][MT_Q][8] keys, sorted, MT_NONE where empty; all: [nq][nc] or null.  grid: (<= MATCH_GRID)
template <unsigned QPT>
__global__ __launch_bounds__(256) void match_kernel(const uint8_t* __restrict__ query, unsigned nq, unsigned q0, const uint8_t* __restrict__ cat,
                                                    uint32_t c_begin, uint32_t c_end, uint32_t nc, uint64_t* __restrict__ part,
                                                    uint32_t* __restrict__ all) {
    constexpr unsigned QT = 16 * QPT, ROWS = QT + MT_C, NLD = ROWS / 16;      // NLD: 16-byte pieces of a slab per thread
    extern __shared__ uint4 s_dyn[];
    uint8_t* s_slab = reinterpret_cast<uint8_t*>(s_dyn);
    uint32_t* s_dist = reinterpret_cast<uint32_t*>(s_dyn);                     // [QT][MT_C], in the slab's place after a tile's last slab
    uint64_t* s_top = reinterpret_cast<uint64_t*>(s_slab + (size_t)ROWS * MT_PITCH);   // [QT][8]
    const unsigned t = threadIdx.x, tc = t & 15, tq = t >> 4, lane = t & 63, wave = t >> 6;
    uint64_t* my_part = part + (size_t)blockIdx.x * MT_Q * MT_TOP;
    for (unsigned i = t; i < QT * MT_TOP; i += 256) s_top[i] = my_part[i];
    const unsigned ntiles = (c_end - c_begin + MT_C - 1) / MT_C;
    for (unsigned tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t c0 = (uint64_t)c_begin + (uint64_t)tile * MT_C;
        uint32_t acc[QPT][8];
#pragma unroll
        for (unsigned f = 0; f < QPT; ++f)
#pragma unroll
            for (unsigned e = 0; e < 8; ++e) acc[f][e] = 0;
        uint4 pf[NLD];
        auto load_slab = [&](unsigned s) {
#pragma unroll
            for (unsigned it = 0; it < NLD; ++it) {
                const unsigned id = it * 256 + t, row = id >> 4, col = id & 15;
                const uint8_t* src = nullptr;
                if (row < QT) { if (q0 + row < nq) src = query + (size_t)(q0 + row) * SIG_BYTES; }
                else if (c0 + (row - QT) < c_end) src = cat + (size_t)(c0 + (row - QT)) * SIG_BYTES;
                pf[it] = make_uint4(0, 0, 0, 0);
                if (src) __builtin_memcpy(&pf[it], src + s * MT_SLAB + col * 16, 16);
            }
        };
        load_slab(0);
        for (unsigned s = 0; s < SIG_BYTES / MT_SLAB; ++s) {
            __syncthreads();                                   // the slab (or the distances of the tile before) is no longer read
#pragma unroll
            for (unsigned it = 0; it < NLD; ++it) {
                const unsigned id = it * 256 + t, row = id >> 4, col = id & 15;
                *reinterpret_cast<uint4*>(s_slab + (size_t)row * MT_PITCH + col * 16) = pf[it];
            }
            __syncthreads();
            if (s + 1 < SIG_BYTES / MT_SLAB) load_slab(s + 1);  // in flight beside the sums below
#pragma unroll 2
            for (unsigned kk = 0; kk < MT_SLAB / 16; ++kk) {
                uint4 cq[QPT], cc[8];
#pragma unroll
                for (unsigned f = 0; f < QPT; ++f) cq[f] = *reinterpret_cast<const uint4*>(s_slab + (size_t)(f * 16 + tq) * MT_PITCH + kk * 16);
#pragma unroll
                for (unsigned e = 0; e < 8; ++e) cc[e] = *reinterpret_cast<const uint4*>(s_slab + (size_t)(QT + e * 16 + tc) * MT_PITCH + kk * 16);
#pragma unroll
                for (unsigned f = 0; f < QPT; ++f)
#pragma unroll
                    for (unsigned e = 0; e < 8; ++e) {
                        uint32_t a = acc[f][e];
                        a = __builtin_amdgcn_sad_u8(cq[f].x, cc[e].x, a);
                        a = __builtin_amdgcn_sad_u8(cq[f].y, cc[e].y, a);
                        a = __builtin_amdgcn_sad_u8(cq[f].z, cc[e].z, a);
                        a = __builtin_amdgcn_sad_u8(cq[f].w, cc[e].w, a);
                        acc[f][e] = a;
                    }
            }
        }
        __syncthreads();
#pragma unroll
        for (unsigned f = 0; f < QPT; ++f)
#pragma unroll
            for (unsigned e = 0; e < 8; ++e) s_dist[(f * 16 + tq) * MT_C + e * 16 + tc] = acc[f][e];
        __syncthreads();
        // wave v owns the rows v, v + 4, ...: their lists are read and written by this wave only
        for (unsigned r = wave; r < QT; r += 4) {
            const unsigned qi = q0 + r;
            if (qi >= nq) break;                               // uniform
            uint64_t key[2];
#pragma unroll
            for (unsigned h = 0; h < 2; ++h) {
                const uint64_t c = c0 + lane + 64 * h;
                const uint32_t dd = s_dist[r * MT_C + lane + 64 * h];
                key[h] = MT_NONE;
                if (c < c_end) {
                    key[h] = ((uint64_t)dd << 32) | c;
                    if (all) all[(size_t)qi * nc + c] = dd;
                }
            }
            uint64_t L[MT_TOP];
#pragma unroll
            for (unsigned i = 0; i < MT_TOP; ++i) L[i] = s_top[r * MT_TOP + i];
            bool changed = false;
            for (unsigned round = 0; round < MT_TOP; ++round) {  // keys come out in ascending order: the ninth cannot pass
                const uint64_t mine = key[0] < key[1] ? key[0] : key[1];
                const bool pass = mine < L[MT_TOP - 1];
                if (__ballot(pass) == 0) break;                 // uniform
                const uint64_t m = wave_min_u64(pass ? mine : MT_NONE);
                if (key[0] == m) key[0] = MT_NONE;
                if (key[1] == m) key[1] = MT_NONE;
#pragma unroll
                for (unsigned i = MT_TOP - 1; i > 0; --i) {      // L'[i] = max(L[i - 1], min(m, L[i])) on a sorted list
                    const uint64_t lo = m < L[i] ? m : L[i];
                    L[i] = L[i - 1] > lo ? L[i - 1] : lo;
                }
                L[0] = m < L[0] ? m : L[0];
                changed = true;
            }
            if (changed && lane == 0) {
#pragma unroll
                for (unsigned i = 0; i < MT_TOP; ++i) s_top[r * MT_TOP + i] = L[i];
            }
        }
    }
    __syncthreads();
    for (unsigned i = t; i < QT * MT_TOP; i += 256) my_part[i] = s_top[i];
}

// One wave per query of the tile: round r takes the smallest key above round r - 1's.  grid: (queries of the tile)
__global__ __launch_bounds__(64) void match_finish_kernel(const uint64_t* __restrict__ part, unsigned q0, unsigned top, uint32_t* __restrict__ index,
                                                          uint32_t* __restrict__ dist) {
    const unsigned r = blockIdx.x, lane = threadIdx.x;
    uint64_t prev = 0;
    for (unsigned round = 0; round < top; ++round) {
        uint64_t m = MT_NONE;
        for (unsigned i = lane; i < MATCH_GRID * MT_TOP; i += 64) {
            const uint64_t k = part[(size_t)(i / MT_TOP) * MT_Q * MT_TOP + r * MT_TOP + i % MT_TOP];
            if ((round == 0 || k > prev) && k < m) m = k;
        }
        m = wave_min_u64(m);
        if (lane == 0) {
            index[(size_t)(q0 + r) * top + round] = (uint32_t)m;            // MT_NONE: 0xFFFFFFFF in both
            dist[(size_t)(q0 + r) * top + round] = (uint32_t)(m >> 32);
        }
        prev = m;
    }
}

namespace host {
namespace {

size_t up(size_t v, size_t a) { return (v + a - 1) / a * a; }

int check_shapes(const ssw_image_shape* shapes, size_t n) {
    for (size_t i = 0; i < n; ++i) {
        const ssw_image_shape& s = shapes[i];
        if (s.w < SIG_GRID || s.h < SIG_GRID || (s.channels != 3 && s.channels != 4)) return SSW_ERR_BAD_ARG;
        if ((uint64_t)s.w * s.channels > 0xFFFFFFFFull) return SSW_ERR_BAD_ARG;
        // a cell's luma sum is kept in 32 bits
        if ((uint64_t)(s.w / SIG_GRID + 1) * (s.h / SIG_GRID + 1) > 0xFFFFFFFFull / 255) return SSW_ERR_UNSUPPORTED;
    }
    return SSW_OK;
}

// enqueues the signatures of n device frames on the context's stream
int signature_enqueue(ssw_ctx* ctx, const void* const* dev_frames, const ssw_image_shape* shapes, size_t n, uint8_t* dev_sigs) {
    hipStream_t st = ctx->stream;
    for (size_t b0 = 0; b0 < n; b0 += SIG_BATCH) {
        const unsigned m = (unsigned)std::min<size_t>(SIG_BATCH, n - b0);
        SigBatch sb{};
        unsigned gsplit = 1;
        double bytes = 0.0;
        for (unsigned i = 0; i < m; ++i) {
            const ssw_image_shape& s = shapes[b0 + i];
            const unsigned split = s.w >= 2048 ? 8u : s.w >= 1024 ? 4u : s.w >= 512 ? 2u : 1u;
            sb.it[i] = SigDev{(const uint8_t*)dev_frames[b0 + i], s.w, s.h, s.channels, split};
            gsplit = std::max(gsplit, split);
            bytes += (double)s.w * s.h * s.channels + SIG_BYTES;
        }
        StageTimer t(ctx, SSW_STAGE_LOCATE, st, bytes);
        signature_kernel<<<dim3(SIG_GRID * gsplit, m), 256, 0, st>>>(sb, gsplit, dev_sigs + b0 * SIG_BYTES);
        SSW_HIP_CHECK(hipGetLastError());
    }
    return SSW_OK;
}

int match_raise_lds_limit() {
    static std::atomic<bool> done[64];
    int dev = 0;
    SSW_HIP_CHECK(hipGetDevice(&dev));
    const bool known = dev >= 0 && dev < 64;
    if (known && done[dev].load(std::memory_order_acquire)) return SSW_OK;
    SSW_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(match_kernel<8>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)match_lds_bytes(128)));
    SSW_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(match_kernel<1>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)match_lds_bytes(16)));
    if (known) done[dev].store(true, std::memory_order_release);
    return SSW_OK;
}

int match_enqueue(ssw_ctx* ctx, const uint8_t* query, size_t nq, const uint8_t* cat, size_t nc, size_t top, uint32_t* index, uint32_t* dist,
                  uint32_t* all) {
    hipStream_t st = ctx->stream;
    SSW_TRY(match_raise_lds_limit());
    SSW_TRY(grow(ctx->catalogue.top8, MT_PART_BYTES));
    uint64_t* part = ctx->catalogue.top8.as<uint64_t>();
    for (size_t q0 = 0; q0 < nq; q0 += MT_Q) {
        const unsigned m = (unsigned)std::min<size_t>(MT_Q, nq - q0);
        // the catalogue once per query tile, the distances of the tile when the caller wants them
        StageTimer t(ctx, SSW_STAGE_LOCATE, st, (double)nc * SIG_BYTES + (double)m * SIG_BYTES + (all ? 4.0 * m * nc : 0.0) + 8.0 * m * top);
        SSW_HIP_CHECK(hipMemsetAsync(part, 0xFF, MT_PART_BYTES, st));
        for (size_t c0 = 0; c0 < nc; c0 += MATCH_CHUNK) {
            const size_t c1 = std::min(nc, c0 + MATCH_CHUNK);
            const unsigned grid = (unsigned)std::min<size_t>(MATCH_GRID, (c1 - c0 + MT_C - 1) / MT_C);
            if (m <= 16)
                match_kernel<1><<<grid, 256, match_lds_bytes(16), st>>>(query, (unsigned)nq, (unsigned)q0, cat, (uint32_t)c0, (uint32_t)c1, (uint32_t)nc, part, all);
            else
                match_kernel<8><<<grid, 256, match_lds_bytes(128), st>>>(query, (unsigned)nq, (unsigned)q0, cat, (uint32_t)c0, (uint32_t)c1, (uint32_t)nc, part, all);
            SSW_HIP_CHECK(hipGetLastError());
        }
        match_finish_kernel<<<m, 64, 0, st>>>(part, (unsigned)q0, (unsigned)top, index, dist);
        SSW_HIP_CHECK(hipGetLastError());
    }
    return SSW_OK;
}

constexpr size_t SIG_GROUP_BYTES = (size_t)256 << 20;      // host form: frames on the device at a time

}  // namespace
}  // namespace host
}  // namespace ssw

extern "C" int ssw_signature_rgb8(ssw_ctx* ctx, const void* const* dev_frames, const ssw_image_shape* shapes, size_t n, uint8_t* dev_sigs) {
    using namespace ssw::host;
    if (!ctx) return SSW_ERR_BAD_ARG;
    if (n == 0) return SSW_OK;
    if (!dev_frames || !shapes || !dev_sigs) return SSW_ERR_BAD_ARG;
    SSW_TRY(check_shapes(shapes, n));
    for (size_t i = 0; i < n; ++i) if (!dev_frames[i]) return SSW_ERR_BAD_ARG;
    CtxGuard g(ctx);
    return signature_enqueue(ctx, dev_frames, shapes, n, dev_sigs);
}

extern "C" int ssw_signature_host_rgb8(ssw_ctx* ctx, const uint8_t* const* host_frames, const ssw_image_shape* shapes, size_t n, uint8_t* host_sigs) {
    using namespace ssw::host;
    if (!ctx) return SSW_ERR_BAD_ARG;
    if (n == 0) return SSW_OK;
    if (!host_frames || !shapes || !host_sigs) return SSW_ERR_BAD_ARG;
    SSW_TRY(check_shapes(shapes, n));
    for (size_t i = 0; i < n; ++i) if (!host_frames[i]) return SSW_ERR_BAD_ARG;
    CtxGuard g(ctx);
    hipStream_t st = ctx->stream;
    auto frame_bytes = [&](size_t i) { return (size_t)shapes[i].w * shapes[i].h * shapes[i].channels; };
    SSW_TRY(grow(ctx->catalogue.sigs, n * ssw::SIG_BYTES));
    uint8_t* sigs = ctx->catalogue.sigs.as<uint8_t>();
    // groups of at most SIG_GROUP_BYTES (one frame's own size if that is more): uploads and kernels are ordered on the
    // context's stream, so the next group's frames overwrite the workspace only behind the kernels that read it
    std::vector<const void*> ptrs;
    std::vector<size_t> offs;
    for (size_t g0 = 0; g0 < n;) {
        size_t g1 = g0, bytes = 0;
        offs.clear();
        while (g1 < n && (g1 == g0 || bytes + frame_bytes(g1) <= SIG_GROUP_BYTES)) { offs.push_back(bytes); bytes += up(frame_bytes(g1++), 256); }
        SSW_TRY(grow(ctx->catalogue.frames, bytes));
        uint8_t* ws = ctx->catalogue.frames.as<uint8_t>();
        ptrs.clear();
        for (size_t i = g0; i < g1; ++i) {
            SSW_TRY(upload(ctx, ws + offs[i - g0], host_frames[i], frame_bytes(i), st));
            ptrs.push_back(ws + offs[i - g0]);
        }
        untimed_work(ctx);
        SSW_TRY(signature_enqueue(ctx, ptrs.data(), shapes + g0, g1 - g0, sigs + g0 * ssw::SIG_BYTES));
        g0 = g1;
    }
    untimed_work(ctx);
    return download(ctx, host_sigs, sigs, n * ssw::SIG_BYTES, st);
}

extern "C" int ssw_signature_match(ssw_ctx* ctx, const uint8_t* dev_query, size_t nq, const uint8_t* dev_catalogue, size_t nc, size_t top,
                                   uint32_t* dev_index, uint32_t* dev_dist, uint32_t* dev_all) {
    using namespace ssw::host;
    if (!ctx || top < 1 || top > ssw::MT_TOP || nc > 0xFFFFFFFFull || nq > 0xFFFFFFFFull) return SSW_ERR_BAD_ARG;
    if (nq == 0) return SSW_OK;
    if (!dev_query || !dev_index || !dev_dist || (nc && !dev_catalogue)) return SSW_ERR_BAD_ARG;
    CtxGuard g(ctx);
    return match_enqueue(ctx, dev_query, nq, dev_catalogue, nc, top, dev_index, dev_dist, dev_all);
}
