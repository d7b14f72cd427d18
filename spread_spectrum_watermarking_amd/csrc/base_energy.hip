// Base-reader pruning, the tail columns' energies as a rigorous upper bound at low precision.
//
// The decide kernel (base_prune.hip) compares G E[v] with T once per column: it needs an upper bound of E[v] = sum_y r32(y, v)^2,
// not E[v] itself, and a bound that is too large only computes a tile more -- "the sums decide what is computed, never a
// value".  The exact f64 row launches therefore run tile column 0 of every class only (the head: columns below 1024 at 4K,
// exact energies); this file's kernel covers the pairs pair0 .. NP - 1 of the eight classes from the same operand planes:
//     x = xh + xl + rx,  b 2^10 = bh + bl + rb      (f16 hi + lo; the operands split in registers, the bases once per shape)
//     a~ = 2^-10 sum_k (xh bh + (xh bl + xl bh))     three v_mfma_f32_16x16x32_f16 per term, f32 accumulators: the hh chain
//                                                    runs through the k-steps, the two correction products of a k-step
//                                                    start from zero and are added once (a VALU add, round to nearest)
// and adds (|a~1 +/- a~2| + err1 + err2)^2 f^2 (rounded up) into energy[frame][v], v the class's column of the pair's output.
// err = S cS + cA per product with S = sum_k |x_k| of the line (accumulated beside the conversion), B = max |basis entry|:
//     cS = B (3 2^-21 + 1.02 n 2^-23) + 2^-23,   n = Kp + Kp / 16 + 16,        cA = 1.01 Kp B 2^-13
//   * 2^-21 |x| + 2^-13 bounds |x - xh - xl|: the f32 rounding of x (2^-24), the f16 rounding of the residual (2^-11 of at most
//     2^-11 (1 + 2^-11) |x|), and both halves flushed or underflowed (2^-14 each) -- times sum |b| <= Kp B: the term cA;
//   * 2^-21 |b| + 2^-23 bounds |b - (bh + bl) 2^-10| the same way (the 2^10 moves the flush range down to 2^-24 per half);
//   * the dropped product xl bl is at most 2^-22 (1 + 2^-10) |x| |b|;
//   * the accumulation: every operation of the hh chain (Kp products' additions, one addition of C per MFMA, one VALU addition
//     of the corrections per k-step) is charged 2^-23 of sum |terms| <= S B (1 + 2^-9) -- a per-operation constant that holds
//     for truncation as well as for rounding, in any order, also for an adder that aligns the 32 terms of an MFMA to the
//     largest and drops what falls off; the corrections' own sums are 2^-10 of that (the + 16);
//   * the f64 launches' own error (Kp 2^-53 S B) and the factor 1.01 / 1.02 of the second-order terms are inside the slack.
// The combination a~1 +/- a~2, the rounding of the exact value to f32, the per-index f32 factor, the squaring and the sum over
// a wave's 16 lines are each one or two f32 operations (2^-24 relative): the value is raised by (1 + 2^-20)^3.  The sum over H
// lines is inside the 2^-5 of G (base_prune.hip).  An operand above the f16 range converts to Inf, and Inf - Inf to NaN: the
// energy comes out Inf / NaN, which the decide kernel reads as "needed".
//
// Block: 512 threads = 8 waves x 16 lines = one 128-line tile (inside ONE frame: the lines are unit-ordered and padded) x up
// to 176 pairs (11 MFMA tiles) of one class: 88 accumulator registers.  Every lane loads its own A fragment from the k-blocked
// plane (64 contiguous bytes per operand and k-step: line = lane & 15, k-block = lane >> 4), so an operand line is read once;
// the basis fragments of a k-step (44 KB) go through LDS, next step's loads in flight behind the MFMAs.
#include <algorithm>
#include <cmath>

#include "dct_pair_common.hpp"

namespace ssw {

namespace {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef float f4 __attribute__((ext_vector_type(4)));

constexpr int BE_THREADS = 512, BE_LINES = 128;
constexpr int BE_NJ = 11;                      // MFMA pair tiles (16 pairs) per block
constexpr float BE_BSCALE = 1024.0f;           // the bases are split as b 2^10
constexpr unsigned BE_FRAG = 64 * 16;          // bytes of one fragment (64 lanes x 8 halves)

struct BeClass {
    const double *x1, *x2;
    const u32x4* y16;
    const float* bmax;
    unsigned NP, Kp, pair0, pm, c1, c2, gsh, e2off, njt;
};
struct BeArgs {
    BeClass c[8];
    unsigned L, lpf, units_valid, W, chunks;
    float factor;
    float* energy;
};

// out: [k-step][basis 0 / 1][hi / lo][pair tile][lane][8 halves]; fragment element e of lane l of pair tile j is
// (pair pair0 + 16 j + (l & 15), k = 32 s + 8 (l >> 4) + e) -- the same k assignment as the operand fragments
__global__ __launch_bounds__(256) void base_energy_split_kernel(const double* __restrict__ y1, const double* __restrict__ y2, unsigned yrows,
                                                                unsigned NP, unsigned Kp, unsigned pair0, unsigned njt, size_t total,
                                                                _Float16* __restrict__ out, float* __restrict__ bmax) {
    const size_t idx = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const unsigned e = (unsigned)(idx & 7u), lane = (unsigned)((idx >> 3) & 63u);
    size_t rest = idx >> 9;
    const unsigned j = (unsigned)(rest % njt);
    rest /= njt;
    const unsigned hl = (unsigned)(rest & 1u), p = (unsigned)((rest >> 1) & 1u), s = (unsigned)(rest >> 2);
    const unsigned pair = pair0 + 16u * j + (lane & 15u), k = 32u * s + 8u * (lane >> 4) + e;
    double b = 0.0;
    if (pair < NP && k < Kp) b = (p ? y2 : y1)[blk_index<double>(pair, k, yrows)];
    const float bf = (float)(b * (double)BE_BSCALE);
    const _Float16 h = (_Float16)bf;
    const float lo = bf - (float)h;
    out[idx] = hl ? (_Float16)lo : h;
    if (hl == 0 && b != 0.0) atomicMax(reinterpret_cast<unsigned*>(bmax), __float_as_uint(fabsf((float)b) * (1.0f + 0x1p-20f)));
}

__global__ __launch_bounds__(BE_THREADS) void prep16_row_energy_kernel(const BeArgs a) {
    __shared__ __attribute__((aligned(16))) u32x4 bsh[4 * BE_NJ * 64];
    __shared__ float eb[2][16 * BE_NJ];
    const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, li = lane & 15u, lq = lane >> 4;
    const unsigned cls = blockIdx.y / a.chunks, chunk = blockIdx.y - cls * a.chunks;
    const BeClass& c = a.c[cls];
    const unsigned j0 = chunk * BE_NJ;
    if (j0 >= c.njt) return;                                   // (block-uniform)
    const unsigned nj = c.njt - j0 < (unsigned)BE_NJ ? c.njt - j0 : (unsigned)BE_NJ;
    const unsigned m0 = blockIdx.x * BE_LINES, L = a.L;
    const unsigned z = m0 / a.lpf, unit = (m0 - z * a.lpf) / 16u + wave;
    const bool wave_valid = unit < a.units_valid && m0 + 16u * wave < L;       // (wave-uniform) padding units carry no image rows
    const unsigned line = m0 + 16u * wave + li < L ? m0 + 16u * wave + li : L - 1u;
    const unsigned nkb = c.Kp / 8u, nsteps = (nkb + 3u) / 4u;
    for (unsigned i = tid; i < 2u * 16u * BE_NJ; i += BE_THREADS) (&eb[0][0])[i] = 0.f;

    // the fragments of k-step s of the block's pair tiles: 4 nj KB, 16 bytes per thread and round
    const unsigned nq = 4u * nj * 64u;
    u32x4 breg[6];
    auto bload = [&](unsigned s) {
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            // (a thread beyond the step's fragments loads the last piece again: the registers stay registers)
            const unsigned q = tid + BE_THREADS * i < nq ? tid + BE_THREADS * i : nq - 1u;
            const unsigned ph = q / (nj * 64u), rem = q - ph * (nj * 64u);
            breg[i] = c.y16[((size_t)(s * 4u + ph) * c.njt + j0) * 64u + rem];
        }
    };
    auto bstore = [&]() {
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            const unsigned q = tid + BE_THREADS * i;
            if (q < nq) bsh[q] = breg[i];
        }
    };
    // this lane's 8 consecutive k of its line, both operands (zero beyond the padded sum length)
    double2 araw[2][4];
    auto aload = [&](unsigned s) {
        const unsigned kb = 4u * s + lq;
#pragma unroll
        for (int o = 0; o < 2; ++o) {
            const double2* src = reinterpret_cast<const double2*>((o ? c.x2 : c.x1) + ((size_t)kb * L + line) * 8u);
#pragma unroll
            for (int i = 0; i < 4; ++i) araw[o][i] = kb < nkb ? src[i] : make_double2(0.0, 0.0);
        }
    };

    f4 acc[2][BE_NJ];
#pragma unroll
    for (int o = 0; o < 2; ++o)
#pragma unroll
        for (int j = 0; j < BE_NJ; ++j) acc[o][j] = (f4){0.f, 0.f, 0.f, 0.f};
    float S[2] = {0.f, 0.f};

    bload(0);
    aload(0);
    bstore();
    __syncthreads();
    for (unsigned s = 0; s < nsteps; ++s) {
        h8 xh[2], xl[2];
#pragma unroll
        for (int o = 0; o < 2; ++o)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float f0 = (float)araw[o][i].x, f1 = (float)araw[o][i].y;
                S[o] += fabsf(f0);
                S[o] += fabsf(f1);
                const _Float16 h0 = (_Float16)f0, h1 = (_Float16)f1;
                xh[o][2 * i] = h0; xh[o][2 * i + 1] = h1;
                xl[o][2 * i] = (_Float16)(f0 - (float)h0); xl[o][2 * i + 1] = (_Float16)(f1 - (float)h1);
            }
        if (s + 1 < nsteps) { bload(s + 1); aload(s + 1); }
        const h8* bf = reinterpret_cast<const h8*>(bsh);
#pragma unroll
        for (int j = 0; j < BE_NJ; ++j) {
            if ((unsigned)j < nj) {                   // (block-uniform)
#pragma unroll
            for (int o = 0; o < 2; ++o) {
                const h8 bh = bf[((2 * o) * nj + j) * 64u + lane], bl = bf[((2 * o + 1) * nj + j) * 64u + lane];
                f4 t = __builtin_amdgcn_mfma_f32_16x16x32_f16(xh[o], bl, (f4){0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
                t = __builtin_amdgcn_mfma_f32_16x16x32_f16(xl[o], bh, t, 0, 0, 0);
                acc[o][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(xh[o], bh, acc[o][j], 0, 0, 0);
                acc[o][j] += t;
            }
            }
        }
        __syncthreads();                          // every wave has read the fragments of step s
        if (s + 1 < nsteps) bstore();
        __syncthreads();
    }

    // S of the line: the four k-groups of a line hold their parts; D map: col = lane & 15 (pair), row = 4 (lane >> 4) + reg (line)
#pragma unroll
    for (int o = 0; o < 2; ++o) { S[o] += __shfl_xor(S[o], 16); S[o] += __shfl_xor(S[o], 32); }
    const float k1 = 1.0f + 0x1p-20f;
    const float B = *c.bmax, n_ops = (float)(c.Kp + c.Kp / 16u + 16u);
    const float cS = (B * (3.0f * 0x1p-21f + 1.02f * n_ops * 0x1p-23f) + 0x1p-23f) * k1;
    const float cA = 1.01f * (float)c.Kp * B * 0x1p-13f * k1 + 1e-30f;
    float err[2][4];
#pragma unroll
    for (int o = 0; o < 2; ++o)
#pragma unroll
        for (int r = 0; r < 4; ++r) err[o][r] = (__shfl(S[o], (int)(4u * lq + r)) * cS + cA) * k1;
    const float fac = fabsf(a.factor) * k1;
#pragma unroll
    for (int j = 0; j < BE_NJ; ++j) {
        if ((unsigned)j >= nj) continue;
        float v1 = 0.f, v2 = 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float a1 = acc[0][j][r] * (1.0f / BE_BSCALE), a2 = acc[1][j][r] * (1.0f / BE_BSCALE);
            float o1, o2, e1, e2;
            if (c.pm) { o1 = fabsf(a1 + a2); o2 = fabsf(a1 - a2); e1 = e2 = err[0][r] + err[1][r]; }
            else      { o1 = fabsf(a1); o2 = fabsf(a2); e1 = err[0][r]; e2 = err[1][r]; }
            const float b1 = (o1 + e1) * k1 * fac, b2 = (o2 + e2) * k1 * fac;
            v1 += b1 * b1 * k1;
            v2 += b2 * b2 * k1;
        }
        v1 += __shfl_xor(v1, 16); v1 += __shfl_xor(v1, 32);
        v2 += __shfl_xor(v2, 16); v2 += __shfl_xor(v2, 32);
        if (wave_valid && lq == 0) {
            atomicAdd(&eb[0][16 * j + li], v1);
            atomicAdd(&eb[1][16 * j + li], v2);
        }
    }
    __syncthreads();
    // one add per (block, output); the order of the adds is free.  Both outputs of every tail pair: the exact epilogue's set
    // of outputs while a class has no pair without a first or a second one (np1 = none, p2lo = 0, pm 0 / 1: the row builder
    // takes this route only then, ssw_pipeline.hip) -- and a superset could only raise the bound.
    if (tid < 2u * 16u * nj) {
        const unsigned o = tid / (16u * nj), pl = tid - o * (16u * nj);
        const unsigned pair = c.pair0 + 16u * j0 + pl;
        if (pair < c.NP && pair >= c.e2off * o) {
            const unsigned e = pair - (o ? c.e2off : 0u);
            const unsigned col = (o ? c.c2 : c.c1) + (e >> c.gsh) * 128u + (e & ((1u << c.gsh) - 1u));
            if (col < a.W) unsafeAtomicAdd(a.energy + (size_t)z * a.W + col, eb[o][pl]);
        }
    }
}

unsigned be_tiles(unsigned NP, unsigned pair0) { return NP > pair0 ? (NP - pair0 + 15u) / 16u : 0u; }
unsigned be_steps(unsigned Kp) { return (Kp / 8u + 3u) / 4u; }
size_t be_frag_bytes(unsigned NP, unsigned Kp, unsigned pair0) { return (size_t)be_steps(Kp) * 4u * be_tiles(NP, pair0) * BE_FRAG; }

}  // namespace

size_t base_energy_split_bytes(unsigned NP, unsigned Kp, unsigned pair0) { return be_frag_bytes(NP, Kp, pair0) + 16; }

int launch_base_energy_split(hipStream_t st, const double* y1, const double* y2, unsigned yrows, unsigned NP, unsigned Kp, unsigned pair0, void* out) {
    const unsigned njt = be_tiles(NP, pair0);
    if (!y1 || !y2 || !out || njt == 0 || Kp == 0 || Kp % 8 != 0 || pair0 % 16 != 0 || yrows < NP) return SSW_ERR_BAD_ARG;
    const size_t frag = be_frag_bytes(NP, Kp, pair0), total = frag / sizeof(_Float16);
    float* bmax = reinterpret_cast<float*>(static_cast<char*>(out) + frag);
    SSW_HIP_CHECK(hipMemsetAsync(bmax, 0, 16, st));
    base_energy_split_kernel<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(y1, y2, yrows, NP, Kp, pair0, njt, total, static_cast<_Float16*>(out), bmax);
    SSW_HIP_CHECK(hipGetLastError());
    return SSW_OK;
}

int launch_base_energy_bound(hipStream_t st, int n_classes, const BaseEnergyClass* cls, size_t n_frames, size_t w, size_t h, size_t lines_per_frame,
                             float factor, float* energy) {
    if (n_frames == 0 || n_classes == 0) return SSW_OK;
    const size_t lines = n_frames * lines_per_frame;
    if (n_classes < 0 || n_classes > 8 || !cls || !energy || lines_per_frame % BE_LINES != 0 || h % 16 != 0 || h > lines_per_frame ||
        lines > 0xFFFFFFFFull || w > 0xFFFFFFull || w % 128 != 0) return SSW_ERR_BAD_ARG;
    BeArgs a;
    unsigned chunks = 0;
    for (int i = 0; i < n_classes; ++i) {
        const BaseEnergyClass& s = cls[i];
        const unsigned njt = be_tiles(s.NP, s.pair0);
        if (!s.x1 || !s.x2 || !s.y16 || njt == 0 || s.Kp == 0 || s.Kp % 8 != 0 || s.pair0 % 16 != 0 || s.gsh > 16 || s.e2off > 1) return SSW_ERR_BAD_ARG;
        if ((unsigned long long)s.Kp * lines * sizeof(double) > 0xFFFFFFFFFFull) return SSW_ERR_BAD_DIMS;
        a.c[i] = BeClass{s.x1, s.x2, static_cast<const u32x4*>(s.y16),
                         reinterpret_cast<const float*>(static_cast<const char*>(s.y16) + be_frag_bytes(s.NP, s.Kp, s.pair0)),
                         s.NP, s.Kp, s.pair0, s.pm, s.c1, s.c2, s.gsh, s.e2off, njt};
        chunks = std::max(chunks, (njt + BE_NJ - 1) / BE_NJ);
    }
    a.L = (unsigned)lines; a.lpf = (unsigned)lines_per_frame; a.units_valid = (unsigned)(h / 16); a.W = (unsigned)w; a.chunks = chunks;
    a.factor = factor; a.energy = energy;
    const dim3 grid((unsigned)(lines / BE_LINES), (unsigned)n_classes * chunks);
    if (grid.y > 65535u) return SSW_ERR_BAD_DIMS;
    prep16_row_energy_kernel<<<grid, BE_THREADS, 0, st>>>(a);
    SSW_HIP_CHECK(hipGetLastError());
    return SSW_OK;
}

}  // namespace ssw
