// HBM-bound pre-passes of the operand-ready GEMMs (dct_pair_f64.hip): they write
// the image operand of a pass once, already folded (forward) or split (inverse), in f64 (every sum exact) and in the
// k-blocked layout (dct_pair_common.hpp).  Also the half bases in that layout.
#include "dct_pair_split.hpp"
#include "dct_pair_colops.hpp"
#include "dct_pair_yiq_load.hpp"

#include <cstdlib>

namespace ssw {

// ---------------------------------------------------------------------------------------------
// Half bases in the k-blocked layout: [Kp / 8][n / 2][8]; row o of parity p holds basis frequency 2 o + p (forward) or the
// inverse's entries of frequencies 2 s + p, zero beyond n / 2.
// ---------------------------------------------------------------------------------------------
__global__ void make_half_basis_blocked_kernel(size_t n, bool inverse, int parity, size_t kpad, double* out) {
    const size_t nh = n / 2, total = nh * kpad;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t o = i / kpad, s = i % kpad;
        double v = 0.0;
        if (s < nh) {
            const size_t freq = inverse ? 2 * s + parity : 2 * o + parity;
            const size_t pos = inverse ? o : s;
            unsigned long long a = (unsigned long long)freq * (2ull * pos + 1ull);
            a %= 4ull * n;
            const double c = cospi((double)a / (double)(2ull * n));
            v = !inverse ? 2.0 * c : (freq == 0 ? 0.25 : 0.5 * c);
        }
        out[blk_index<double>(o, (unsigned)s, nh)] = v;
    }
}

size_t dct_pair_kpad(size_t n) { return pair_kpad(n); }

int launch_make_half_basis_blocked(hipStream_t st, size_t n, bool inverse, int parity, double* out) {
    const size_t kp = pair_kpad(n), total = (n / 2) * kp;
    const unsigned blocks = (unsigned)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    make_half_basis_blocked_kernel<<<blocks ? blocks : 1, 256, 0, st>>>(n, inverse, parity, kp, out);
    SSW_HIP_CHECK(hipGetLastError());
    return SSW_OK;
}

// ---------------------------------------------------------------------------------------------
// Split odd half.  The odd frequencies of a length-N transform are a DCT-IV of the M = N/2 differences d[n]:
//   X[k] = sum_{n<M} d[n] cos(pi (2k+1)(2n+1) / (4M)),  k < M           (frequency 2k+1; inverse: the same sum with the
//                                                                         roles of k and n exchanged -- the matrix is symmetric)
// Pairing n with M-1-n and splitting the angle of an even k = 2j into pi j (2n+1)/M + psi_n, psi_n = pi (2n+1)/(4M):
//   a[n] =  d[n] cos psi_n + d[M-1-n] sin psi_n,   b[n] = -d[n] sin psi_n + d[M-1-n] cos psi_n        (n < M/2: a rotation)
//   A[j] = sum_n a[n] cos(pi j (2n+1)/M),  B[j] = sum_n b[n] sin(pi j (2n+1)/M)                       (j = 0 .. M/2)
//   X[2j] = A[j] + B[j],   X[2j-1] = A[j] - B[j]
// A is a DCT-II and B a DST-II of length M/2; both fold once more (n <-> M/2-1-n, exact additions):
//   j = 2i   :  A = sum_{n<M/4} (a[n] + a[M/2-1-n]) cos(..),   B = sum (b[n] - b[M/2-1-n]) sin(..)    operands AS, BD
//   j = 2i+1 :  A = sum_{n<M/4} (a[n] - a[M/2-1-n]) cos(..),   B = sum (b[n] + b[M/2-1-n]) sin(..)    operands AD, BS
// i.e. two GEMM launches with K = M/4 = N/8 and N/8 (+1) output pairs instead of one with K = N/2 and N/4 pairs:
// a quarter of the multiply-adds.  The only inexact step before the MFMA sums is the rotation (two f64 products and
// one sum per operand element, relative error 2^-52 of |d|): the folded operands of the other launches stay exact.
// Bases, k-blocked like the half bases: rows i of scale * cos / sin(2 pi j (2n+1) / N), j = 2i (E, N/8 + 1 rows) or
// 2i + 1 (O, N/8 rows), n < N/8; scale 2 forward, 1/2 inverse as in make_half_basis_blocked_kernel.
// ---------------------------------------------------------------------------------------------
__global__ void make_split_basis_blocked_kernel(size_t n, bool inverse, int which /*0 cosE, 1 sinE, 2 cosO, 3 sinO, 4 sinE with row 0 := row n/8*/, size_t kpad,
                                                size_t rows, double* out) {
    const size_t ktrue = n / 8, total = rows * kpad;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t o = i / kpad, s = i % kpad;
        double v = 0.0;
        if (s < ktrue) {
            const unsigned long long j = (which & 2) ? 2ull * o + 1ull : (which == 4 && o == 0) ? 2ull * (n / 8) : 2ull * o;
            const unsigned long long a = (j * (2ull * s + 1ull)) % (unsigned long long)n;       // angle 2 pi a / n
            const double arg = (double)(2ull * a) / (double)n;
            const double c = ((which & 1) || which == 4) ? sinpi(arg) : cospi(arg);
            v = (inverse ? 0.5 : 2.0) * c;
        }
        out[blk_index<double>(o, (unsigned)s, rows)] = v;
    }
}
// rotation table of a length-n axis: [0 .. n/4) cos psi, [n/4 .. n/2) sin psi, psi = pi (2 m + 1) / (2 n)
__global__ void make_rot_table_kernel(size_t n, double* out) {
    const size_t q = n / 4;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < q; i += (size_t)gridDim.x * blockDim.x) {
        const double arg = (double)(2ull * i + 1ull) / (double)(2ull * n);
        out[i] = cospi(arg);
        out[q + i] = sinpi(arg);
    }
}

size_t dct_pair_split_kpad(size_t len) { return pair_kpad(len / 4); }
// doubles in the four split planes of a pass over n frames (the larger of the row and the column pass)
size_t dct_pair_split_elems(size_t n_frames, size_t w, size_t h) {
    const size_t a = n_frames * h * dct_pair_split_kpad(w), b = n_frames * w * dct_pair_split_kpad(h);
    return 4 * (a > b ? a : b);
}
size_t dct_pair_split_basis_rows(size_t len, int which) { return (which & 2) ? len / 8 : len / 8 + 1; }      // which 4 like 1

int launch_make_split_basis_blocked(hipStream_t st, size_t n, bool inverse, int which, double* out) {
    const size_t kp = dct_pair_split_kpad(n), rows = dct_pair_split_basis_rows(n, which), total = rows * kp;
    const unsigned blocks = (unsigned)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    make_split_basis_blocked_kernel<<<blocks ? blocks : 1, 256, 0, st>>>(n, inverse, which, kp, rows, out);
    SSW_HIP_CHECK(hipGetLastError());
    return SSW_OK;
}
int launch_make_rot_table(hipStream_t st, size_t n, double* out) {
    make_rot_table_kernel<<<(unsigned)((n / 4 + 255) / 256 ? (n / 4 + 255) / 256 : 1), 256, 0, st>>>(n, out);
    SSW_HIP_CHECK(hipGetLastError());
    return SSW_OK;
}

// Rotation + fold of an odd operand plane P ([Kp / 8][L][8], positions n < M = len/2) into the four split planes
// ([K8 / 8][L][8], K8 = kpad(len/4), zero padded): one thread = one line x 8 consecutive e (one 64-byte piece of each
// output plane); consecutive threads take consecutive lines, so every piece access of a wave is one contiguous run.
// ALIGNED: M/2 is a multiple of 8 and the mirrored positions are whole pieces too (16-byte loads); otherwise the
// mirrored elements are fetched one by one.
template <bool ALIGNED>
__global__ __launch_bounds__(256) void pair_rotate_kernel(const double* __restrict__ P, const double* __restrict__ rot,
                                                         double* __restrict__ AS, double* __restrict__ BD,
                                                         double* __restrict__ AD, double* __restrict__ BS,
                                                         unsigned L, unsigned M, unsigned K8, unsigned line_blocks) {
    const unsigned line = (blockIdx.x % line_blocks) * 256 + threadIdx.x;
    const unsigned e0 = (blockIdx.x / line_blocks) * 8;
    if (line >= L || e0 >= K8) return;
    const unsigned Mh = M / 2, Mq = M / 4;
    double as[8], bd[8], ad[8], bs[8];
    auto ld = [&](unsigned pos) { return P[blk_index<double>(line, pos, L)]; };
    double d0[8], d1[8], d2[8], d3[8];          // d[e], d[M/2-1-e], d[M/2+e], d[M-1-e]
    if (ALIGNED && e0 + 8 <= Mq) {
        const double* p0 = P + blk_index<double>(line, e0, L);
        const double* p1 = P + blk_index<double>(line, Mh - 8 - e0, L);
        const double* p2 = P + blk_index<double>(line, Mh + e0, L);
        const double* p3 = P + blk_index<double>(line, M - 8 - e0, L);
#pragma unroll
        for (int i = 0; i < 8; i += 2) {
            const f64x2 v0 = *reinterpret_cast<const f64x2*>(p0 + i), v1 = *reinterpret_cast<const f64x2*>(p1 + i);
            const f64x2 v2 = *reinterpret_cast<const f64x2*>(p2 + i), v3 = *reinterpret_cast<const f64x2*>(p3 + i);
            d0[i] = v0[0]; d0[i + 1] = v0[1];
            d1[7 - i] = v1[0]; d1[6 - i] = v1[1];
            d2[i] = v2[0]; d2[i + 1] = v2[1];
            d3[7 - i] = v3[0]; d3[6 - i] = v3[1];
        }
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const unsigned e = e0 + i;
            const bool ok = e < Mq;
            d0[i] = ok ? ld(e) : 0.0;
            d1[i] = ok ? ld(Mh - 1 - e) : 0.0;
            d2[i] = ok ? ld(Mh + e) : 0.0;
            d3[i] = ok ? ld(M - 1 - e) : 0.0;
        }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const unsigned e = e0 + i;
        const unsigned ec = e < Mq ? e : 0, em = Mh - 1 - ec;          // n = e and its mirror n' = M/2 - 1 - e
        const double c = rot[ec], s = rot[Mh + ec], cm = rot[em], sm = rot[Mh + em];
        const double a = d0[i] * c + d3[i] * s, b = d3[i] * c - d0[i] * s;                 // n: partner M-1-n
        const double am = d1[i] * cm + d2[i] * sm, bm = d2[i] * cm - d1[i] * sm;           // n': partner M-1-n' = M/2 + e
        const bool ok = e < Mq;
        as[i] = ok ? a + am : 0.0;
        ad[i] = ok ? a - am : 0.0;
        bs[i] = ok ? b + bm : 0.0;
        bd[i] = ok ? b - bm : 0.0;
    }
    const size_t at = blk_index<double>(line, e0, L);
#pragma unroll
    for (int i = 0; i < 8; i += 2) {
        *reinterpret_cast<f64x2*>(AS + at + i) = (f64x2){as[i], as[i + 1]};
        *reinterpret_cast<f64x2*>(BD + at + i) = (f64x2){bd[i], bd[i + 1]};
        *reinterpret_cast<f64x2*>(AD + at + i) = (f64x2){ad[i], ad[i + 1]};
        *reinterpret_cast<f64x2*>(BS + at + i) = (f64x2){bs[i], bs[i + 1]};
    }
}

// P: the odd operand plane of a length-`len` axis (kpad(len) wide, `lines` lines) -> sp: four consecutive planes
// AS | BD | AD | BS of lines * K8 doubles each
int launch_dct_pair_rotate(hipStream_t st, const double* p, const double* rot, double* sp, size_t lines, size_t len) {
    if (lines == 0) return SSW_OK;
    if (lines > 0xFFFFFFFFull || len % 8 != 0) return SSW_ERR_BAD_DIMS;
    const unsigned L = (unsigned)lines, M = (unsigned)(len / 2), K8 = (unsigned)dct_pair_split_kpad(len);
    const unsigned line_blocks = (L + 255) / 256;
    const unsigned long long nblk = (unsigned long long)line_blocks * (K8 / 8);
    if (nblk > 0x7FFFFFFFull) return SSW_ERR_BAD_DIMS;
    const size_t plane = (size_t)L * K8;
    if ((M / 2) % 8 == 0) pair_rotate_kernel<true><<<(unsigned)nblk, 256, 0, st>>>(p, rot, sp, sp + plane, sp + 2 * plane, sp + 3 * plane, L, M, K8, line_blocks);
    else                  pair_rotate_kernel<false><<<(unsigned)nblk, 256, 0, st>>>(p, rot, sp, sp + plane, sp + 2 * plane, sp + 3 * plane, L, M, K8, line_blocks);
    SSW_HIP_CHECK(hipGetLastError());
    return SSW_OK;
}

// ---------------------------------------------------------------------------------------------
// Pre-passes (HBM-bound): f32 plane -> the f64 operand planes of the pass, k-blocked.
// One folding level:   forward  O1 = S, O2 = D;   inverse  O1 = E (even coefficients), O2 = O (odd)
// ---------------------------------------------------------------------------------------------
// Row pass: line = image row, k along the row.  Block = 32 lines x 32 k; thread = 4 consecutive k of
// one line: 128-byte read runs per line, 512-byte write runs per k-block.
template <bool INVERSE>
__global__ __launch_bounds__(256) void pair_prep_rows_kernel(const float* __restrict__ X, double* __restrict__ O1,
                                                            double* __restrict__ O2, unsigned rows, unsigned W, unsigned Kp,
                                                            unsigned tiles_k) {
    const unsigned Nh = W / 2;
    const unsigned s = (blockIdx.x % tiles_k) * 32 + (threadIdx.x & 7) * 4;
    const unsigned row = (blockIdx.x / tiles_k) * 32 + (threadIdx.x >> 3);
    if (row >= rows || s >= Kp) return;
    f64x4 a = {0, 0, 0, 0}, b = {0, 0, 0, 0};
    if (s < Nh) {                                                 // Nh % 4 == 0
        const float* x = X + (size_t)row * W;
        if (!INVERSE) {
            const f32x4 u = *reinterpret_cast<const f32x4*>(x + s);
            const f32x4 v = *reinterpret_cast<const f32x4*>(x + (W - 4 - s));
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                a[e] = (double)u[e] + (double)v[3 - e];
                b[e] = (double)u[e] - (double)v[3 - e];
            }
        } else {
            const f32x4 u = *reinterpret_cast<const f32x4*>(x + 2 * s);
            const f32x4 v = *reinterpret_cast<const f32x4*>(x + 2 * s + 4);
            a = (f64x4){(double)u[0], (double)u[2], (double)v[0], (double)v[2]};
            b = (f64x4){(double)u[1], (double)u[3], (double)v[1], (double)v[3]};
        }
    }
    *reinterpret_cast<f64x4*>(O1 + blk_index<double>(row, s, rows)) = a;
    *reinterpret_cast<f64x4*>(O2 + blk_index<double>(row, s, rows)) = b;
}

// Column pass: line = (frame, column), k along the image rows: fold / split + transpose through LDS.
// Block tile: 32 k x 64 columns; written as 4 KB runs (64 lines x one 64-byte k-block piece).
template <bool INVERSE>
__global__ __launch_bounds__(256) void pair_prep_cols_kernel(const float* __restrict__ IN, double* __restrict__ O1,
                                                            double* __restrict__ O2, unsigned W, unsigned H, unsigned Kp,
                                                            unsigned n_frames, unsigned tiles_k, unsigned tiles_c) {
    __shared__ double s1[64][33];
    __shared__ double s2[64][33];
    const unsigned Hh = H / 2;
    const unsigned z = blockIdx.x / (tiles_k * tiles_c);
    const unsigned tt = blockIdx.x % (tiles_k * tiles_c);
    const unsigned k0 = (tt % tiles_k) * 32, c0 = (tt / tiles_k) * 64;
    const float* __restrict__ P = IN + (size_t)z * H * W;
    const unsigned tid = threadIdx.x;
    {
        const unsigned kr = tid >> 4, cq = (tid & 15) * 4;       // 16 k-rows per sweep, 4 columns per thread
        unsigned c = c0 + cq;
        c = c + 4 <= W ? c : W - 4;                               // W % 4 == 0; duplicates are never written out
#pragma unroll
        for (int sw = 0; sw < 2; ++sw) {
            const unsigned kl = kr + 16 * sw, k = k0 + kl;
            f32x4 u = {0.f, 0.f, 0.f, 0.f}, v = {0.f, 0.f, 0.f, 0.f};
            if (k < Hh) {
                const unsigned ra = INVERSE ? 2 * k : k, rb = INVERSE ? 2 * k + 1 : H - 1 - k;
                u = *reinterpret_cast<const f32x4*>(P + (size_t)ra * W + c);
                v = *reinterpret_cast<const f32x4*>(P + (size_t)rb * W + c);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                s1[cq + e][kl] = INVERSE ? (double)u[e] : (double)u[e] + (double)v[e];
                s2[cq + e][kl] = INVERSE ? (double)v[e] : (double)u[e] - (double)v[e];
            }
        }
    }
    __syncthreads();
    {
        const unsigned cl = tid & 63, kq = (tid >> 6) * 8;        // one 64-byte k-block piece of one column per thread
        const unsigned c = c0 + cl;
        if (c < W && k0 + kq < Kp) {                              // Kp % 8 == 0
            const size_t at = blk_index<double>((size_t)z * W + c, k0 + kq, (size_t)n_frames * W);
#pragma unroll
            for (int e = 0; e < 8; e += 2) {
                *reinterpret_cast<f64x2*>(O1 + at + e) = (f64x2){s1[cl][kq + e], s1[cl][kq + e + 1]};
                *reinterpret_cast<f64x2*>(O2 + at + e) = (f64x2){s2[cl][kq + e], s2[cl][kq + e + 1]};
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Two-level pre-passes: f32 plane -> (SS, SD, D) forward / (EE, EO, O) inverse in one sweep
// (12 B/px of HBM traffic; a separate second-level pass over S would make it 20).  The forward ROW pass reads any RowSrc:
// straight from the RGB frame (rgb -> Y, yiq.rs:177-186, formed on the fly) the Y plane is never written and re-read as f32
// (8 B/px less HBM traffic per transform); I and Q planes are written for the writer, not for readers.
//   forward, q < n/4:  S[q] = x[q] + x[n-1-q],  S' = x[n/2-1-q] + x[n/2+q];  SS = S + S',  SD = S - S'
//                      D[q] = x[q] - x[n-1-q],  D[n/2-1-q] = x[n/2-1-q] - x[n/2+q]
//   inverse, q < n/4:  EE[q] = c[4q],  EO[q] = c[4q+2],  O[2q] = c[4q+1],  O[2q+1] = c[4q+3]
// Q1, Q2: kq = pair_kpad(n/2) wide; P: kp = pair_kpad(n) wide; k-blocked, zero padded.
// ---------------------------------------------------------------------------------------------
template <bool INVERSE, RowSrc SRC, bool WITH_IQ>
__global__ __launch_bounds__(256) void pair_prep4_rows_kernel(const void* __restrict__ SRCP, double* __restrict__ Q1,
                                                             double* __restrict__ Q2, double* __restrict__ P,
                                                             float* __restrict__ IP, float* __restrict__ QP,
                                                             unsigned rows, unsigned W, unsigned Kq, unsigned Kp,
                                                             unsigned tiles_q) {
    static_assert(!INVERSE || SRC == RowSrc::Plane, "an inverse pass reads a coefficient plane");
    const unsigned Nh = W / 2, Nq = W / 4;
    const unsigned q = (blockIdx.x % tiles_q) * 32 + (threadIdx.x & 7) * 4;
    const unsigned row = (blockIdx.x / tiles_q) * 32 + (threadIdx.x >> 3);
    if (row >= rows || q >= Kq) return;
    f64x4 a1 = {0, 0, 0, 0}, a2 = {0, 0, 0, 0};
    if (q < Nq) {                                                 // Nq % 4 == 0
        if (!INVERSE) {
            const unsigned pos[4] = {q, Nh - 4 - q, Nh + q, W - 4 - q};
            f32x4 y[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) y[u] = load_row_y4<SRC, WITH_IQ>(SRCP, IP, QP, row, W, pos[u]);
            const f32x4 a = y[0], b = y[1], c = y[2], d = y[3];
            f64x4 dn, dm;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const double s1 = (double)a[e] + (double)d[3 - e], s2 = (double)b[3 - e] + (double)c[e];
                a1[e] = s1 + s2;
                a2[e] = s1 - s2;
                dn[e] = (double)a[e] - (double)d[3 - e];
                dm[3 - e] = (double)b[3 - e] - (double)c[e];
            }
            *reinterpret_cast<f64x4*>(P + blk_index<double>(row, q, rows)) = dn;
            *reinterpret_cast<f64x4*>(P + blk_index<double>(row, Nh - 4 - q, rows)) = dm;
        } else {
            const float* x = static_cast<const float*>(SRCP) + (size_t)row * W;
            f32x4 c[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) c[e] = *reinterpret_cast<const f32x4*>(x + 4 * (q + e));
#pragma unroll
            for (int e = 0; e < 4; ++e) { a1[e] = (double)c[e][0]; a2[e] = (double)c[e][2]; }
            double* o = P + blk_index<double>(row, 2 * q, rows);           // 2 q is a multiple of 8: one whole k-block piece
            *reinterpret_cast<f64x4*>(o) = (f64x4){(double)c[0][1], (double)c[0][3], (double)c[1][1], (double)c[1][3]};
            *reinterpret_cast<f64x4*>(o + 4) = (f64x4){(double)c[2][1], (double)c[2][3], (double)c[3][1], (double)c[3][3]};
        }
    }
    *reinterpret_cast<f64x4*>(Q1 + blk_index<double>(row, q, rows)) = a1;
    *reinterpret_cast<f64x4*>(Q2 + blk_index<double>(row, q, rows)) = a2;
    if (q == 0)
        for (unsigned z = Nh; z < Kp; z += 4) *reinterpret_cast<f64x4*>(P + blk_index<double>(row, z, rows)) = (f64x4){0, 0, 0, 0};
}

// Column pass: lines = (frame, column); block tile 32 q x 32 columns, transposed through LDS and
// written as 2 KB runs (32 lines x one 64-byte k-block piece).
template <bool INVERSE>
__global__ __launch_bounds__(256) void pair_prep4_cols_kernel(const float* __restrict__ IN, double* __restrict__ Q1,
                                                             double* __restrict__ Q2, double* __restrict__ P,
                                                             unsigned W, unsigned H, unsigned Kq, unsigned Kp,
                                                             unsigned n_frames, unsigned tiles_q, unsigned tiles_c) {
    __shared__ double sA[32][33], sB[32][33], sC[32][33], sD[32][33];
    const unsigned Hh = H / 2, Hq = H / 4;
    const unsigned z = blockIdx.x / (tiles_q * tiles_c);
    const unsigned tt = blockIdx.x % (tiles_q * tiles_c);
    const unsigned q0 = (tt % tiles_q) * 32, c0 = (tt / tiles_q) * 32;
    const float* __restrict__ Pz = IN + (size_t)z * H * W;
    const unsigned tid = threadIdx.x;
    {
        const unsigned qr = tid >> 3, cq = (tid & 7) * 4, q = q0 + qr;
        unsigned c = c0 + cq;
        c = c + 4 <= W ? c : W - 4;                               // W % 4 == 0; duplicates are never written out
        f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = a, cc = a, d = a;
        if (q < Hq) {
            const unsigned ra = INVERSE ? 4 * q : q, rb = INVERSE ? 4 * q + 2 : Hh - 1 - q;
            const unsigned rc = INVERSE ? 4 * q + 1 : Hh + q, rd = INVERSE ? 4 * q + 3 : H - 1 - q;
            a = *reinterpret_cast<const f32x4*>(Pz + (size_t)ra * W + c);
            b = *reinterpret_cast<const f32x4*>(Pz + (size_t)rb * W + c);
            cc = *reinterpret_cast<const f32x4*>(Pz + (size_t)rc * W + c);
            d = *reinterpret_cast<const f32x4*>(Pz + (size_t)rd * W + c);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (!INVERSE) {
                const double s1 = (double)a[e] + (double)d[e], s2 = (double)b[e] + (double)cc[e];
                sA[cq + e][qr] = s1 + s2;
                sB[cq + e][qr] = s1 - s2;
                sC[cq + e][qr] = (double)a[e] - (double)d[e];        // D[q]
                sD[cq + e][qr] = (double)b[e] - (double)cc[e];       // D[H/2-1-q]
            } else {
                sA[cq + e][qr] = (double)a[e];                        // EE[q]
                sB[cq + e][qr] = (double)b[e];                        // EO[q]
                sC[cq + e][qr] = (double)cc[e];                       // O[2q]
                sD[cq + e][qr] = (double)d[e];                        // O[2q+1]
            }
        }
    }
    __syncthreads();
    {
        const unsigned cl = tid & 31, kq = (tid >> 5) * 4;         // 4 consecutive q of one column per thread
        const unsigned c = c0 + cl, q = q0 + kq;
        if (c < W && q < Kq) {
            const size_t line = (size_t)z * W + c, lines = (size_t)n_frames * W;
            *reinterpret_cast<f64x4*>(Q1 + blk_index<double>(line, q, lines)) = (f64x4){sA[cl][kq], sA[cl][kq + 1], sA[cl][kq + 2], sA[cl][kq + 3]};
            *reinterpret_cast<f64x4*>(Q2 + blk_index<double>(line, q, lines)) = (f64x4){sB[cl][kq], sB[cl][kq + 1], sB[cl][kq + 2], sB[cl][kq + 3]};
            if (q < Hq && q + 4 > Hq) {                             // H/4 not a multiple of 4: the last quad is partial
                for (unsigned e = 0; q + e < Hq; ++e) {
                    if (!INVERSE) {
                        P[blk_index<double>(line, q + e, lines)] = sC[cl][kq + e];
                        P[blk_index<double>(line, Hh - 1 - (q + e), lines)] = sD[cl][kq + e];
                    } else {
                        P[blk_index<double>(line, 2 * (q + e), lines)] = sC[cl][kq + e];
                        P[blk_index<double>(line, 2 * (q + e) + 1, lines)] = sD[cl][kq + e];
                    }
                }
            } else if (q < Hq) {
                if (!INVERSE) {
                    *reinterpret_cast<f64x4*>(P + blk_index<double>(line, q, lines)) = (f64x4){sC[cl][kq], sC[cl][kq + 1], sC[cl][kq + 2], sC[cl][kq + 3]};
                    *reinterpret_cast<f64x4*>(P + blk_index<double>(line, Hh - 4 - q, lines)) = (f64x4){sD[cl][kq + 3], sD[cl][kq + 2], sD[cl][kq + 1], sD[cl][kq]};
                } else {
                    double* o = P + blk_index<double>(line, 2 * q, lines);
                    *reinterpret_cast<f64x4*>(o) = (f64x4){sC[cl][kq], sD[cl][kq], sC[cl][kq + 1], sD[cl][kq + 1]};
                    *reinterpret_cast<f64x4*>(o + 4) = (f64x4){sC[cl][kq + 2], sD[cl][kq + 2], sC[cl][kq + 3], sD[cl][kq + 3]};
                }
            }
            if (q == 0)
                for (unsigned zz = Hh; zz < Kp; zz += 4) *reinterpret_cast<f64x4*>(P + blk_index<double>(line, zz, lines)) = (f64x4){0, 0, 0, 0};
        }
    }
}
// ---------------------------------------------------------------------------------------------
// Three folding levels on a forward row pass (n % 32 == 0): the even part of the even part folds once
// more.  With S = fold(x) (length n/2), SS = fold(S) (n/4), SSS = fold(SS) (n/8):
//   R1 = SSS, R2 = SS - mirror (-> frequencies 0, 4 mod 8; width kpad(n/4))
//   M  = S - mirror            (-> frequencies 2 mod 4;    width kpad(n/2))
//   P  = x - mirror            (-> odd frequencies;        width kpad(n))
// One thread = one quad e < n/8 of one line: it reads the 8 quads of x that meet in it.  The source is
// any RowSrc (ssw_internal.hpp; dct_pair_yiq_load.hpp: Y formed on the fly, I / Q written for the writer).
// ---------------------------------------------------------------------------------------------
template <RowSrc SRC, bool WITH_IQ>
__global__ __launch_bounds__(256) void pair_prep8_rows_kernel(const void* __restrict__ SRCP, double* __restrict__ R1,
                                                             double* __restrict__ R2, double* __restrict__ M, double* __restrict__ P,
                                                             float* __restrict__ IP, float* __restrict__ QP,
                                                             unsigned rows, unsigned W, unsigned K8, unsigned Kq, unsigned Kp,
                                                             unsigned tiles_e) {
    const unsigned Nh = W / 2, Nq = W / 4, Ne = W / 8;
    const unsigned e0 = (blockIdx.x % tiles_e) * 32 + (threadIdx.x & 7) * 4;
    const unsigned row = (blockIdx.x / tiles_e) * 32 + (threadIdx.x >> 3);
    if (row >= rows || e0 >= K8) return;
    f64x4 r1 = {0, 0, 0, 0}, r2 = {0, 0, 0, 0};
    if (e0 < Ne) {                                                // Ne % 4 == 0
        // quads of x, ascending positions; quad u mirrors quad 7 - u
        const unsigned pos[8] = {e0, Nq - 4 - e0, Nq + e0, Nh - 4 - e0, Nh + e0, 3 * Nq - 4 - e0, 3 * Nq + e0, W - 4 - e0};
        f32x4 x[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) x[u] = load_row_y4<SRC, WITH_IQ>(SRCP, IP, QP, row, W, pos[u]);
        // level 1: S and D1 at the positions of quads 0..3 (their mirrors are quads 7..4, reversed)
        f64x4 S[4], D1[4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                S[u][i] = (double)x[u][i] + (double)x[7 - u][3 - i];
                D1[u][i] = (double)x[u][i] - (double)x[7 - u][3 - i];
            }
#pragma unroll
        for (int u = 0; u < 4; ++u) *reinterpret_cast<f64x4*>(P + blk_index<double>(row, pos[u], rows)) = D1[u];
        // level 2 on S (length n/2): quad 0 mirrors quad 3, quad 1 mirrors quad 2
        f64x4 SS[2], D2[2];
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                SS[u][i] = S[u][i] + S[3 - u][3 - i];
                D2[u][i] = S[u][i] - S[3 - u][3 - i];
            }
#pragma unroll
        for (int u = 0; u < 2; ++u) *reinterpret_cast<f64x4*>(M + blk_index<double>(row, pos[u], rows)) = D2[u];
        // level 3 on SS (length n/4): quad 0 mirrors quad 1
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            r1[i] = SS[0][i] + SS[1][3 - i];
            r2[i] = SS[0][i] - SS[1][3 - i];
        }
    }
    *reinterpret_cast<f64x4*>(R1 + blk_index<double>(row, e0, rows)) = r1;
    *reinterpret_cast<f64x4*>(R2 + blk_index<double>(row, e0, rows)) = r2;
    if (e0 == 0) {
        for (unsigned z = Nh; z < Kp; z += 4) *reinterpret_cast<f64x4*>(P + blk_index<double>(row, z, rows)) = (f64x4){0, 0, 0, 0};
        for (unsigned z = Nq; z < Kq; z += 4) *reinterpret_cast<f64x4*>(M + blk_index<double>(row, z, rows)) = (f64x4){0, 0, 0, 0};
    }
}

// ---------------------------------------------------------------------------------------------
// "Deep" forward pre-pass of a row pass (n % 64 == 0): everything the five GEMM launches of the pass consume, from one
// sweep over the source (see "Split odd half" above):
//   level 1   S = x + mirror, D = x - mirror                          (length n/2)
//   D   -> rotation + fold -> AS, BD, AD, BS        (n/8 each)        odd frequencies          (launches E, O)
//   level 2   SS = S + mirror, SD = S - mirror                        (length n/4)
//   SD  -> rotation + fold -> AS2, BD2, AD2, BS2    (n/16 each)       frequencies 2 mod 4      (launches E', O')
//   level 3   R1 = SS + mirror, R2 = SS - mirror    (n/8 each)        frequencies 0 and 4 mod 8 (launch R)
// One thread = 4 consecutive e < n/16 of one line: the 16 quads of x that meet in them (quad u mirrors quad 15 - u).
// Planes are k-blocked, K8 = kpad(n/4) (>= n/8) and K16 = kpad(n/8) (>= n/16) wide, zero padded.
// ---------------------------------------------------------------------------------------------
template <RowSrc SRC, bool WITH_IQ>
__global__ __launch_bounds__(256) void pair_prep16_rows_kernel(const void* __restrict__ SRCP, DeepPlanes dp,
                                                              const double* __restrict__ rot1, const double* __restrict__ rot2,
                                                              const double* __restrict__ rot3,
                                                              float* __restrict__ IP, float* __restrict__ QP,
                                                              unsigned rows, unsigned W, unsigned K8, unsigned K16, unsigned tiles_e, unsigned efold,
                                                              unsigned unit_h, unsigned unit_hup) {
    const unsigned Nh = W / 2, Nq = W / 4, N8 = W / 8, N16 = W / 16;
    const unsigned e0 = (blockIdx.x % tiles_e) * 32 + (threadIdx.x & 7) * 4;
    // operand line of this thread, and the image row it holds (fused_line_row, dct_pair_colops.hpp: natural order, or the fused
    // forward transform's unit order -- a block's 32 lines are then 32 rows of sixteen regions of the frame: the reads are 384-byte
    // runs per row either way, the stores stay 2 KB runs).  `rows` counts operand lines (the planes' line stride).
    const unsigned line = (blockIdx.x / tiles_e) * 32 + (threadIdx.x >> 3);
    if (line >= rows || e0 >= K16) return;
    bool pad_line;
    const unsigned row = fused_line_row(line, unit_h, unit_hup, pad_line);
    double* AD = static_cast<double*>(dp.ad); double* BS = static_cast<double*>(dp.bs);
    double* R1 = static_cast<double*>(dp.r1); double* R2 = static_cast<double*>(dp.r2);
    double* AS2 = static_cast<double*>(dp.as2); double* BD2 = static_cast<double*>(dp.bd2); double* AD2 = static_cast<double*>(dp.ad2); double* BS2 = static_cast<double*>(dp.bs2);
    auto put = [&](double* plane, unsigned k, const f64x4& v) { *reinterpret_cast<f64x4*>(plane + blk_index<double>(line, k, rows)) = v; };
    const f64x4 zero = {0, 0, 0, 0};
    if (e0 >= N16 || pad_line) {                                  // padding of the n/16-wide planes; lines of the padding units
        put(AS2, e0, zero); put(BD2, e0, zero); put(AD2, e0, zero); put(BS2, e0, zero);
        if (efold) {
            void* const l2[12] = {dp.asp, dp.asm_, dp.bdp, dp.bdm, dp.oap, dp.obp, dp.oam, dp.obm, dp.r1p, dp.r1m, dp.r2a, dp.r2b};
#pragma unroll
            for (int a = 0; a < 12; ++a) put(static_cast<double*>(l2[a]), e0, zero);
        }
        return;
    }
    // quads of x, ascending positions inside a quad
    const unsigned pos[8] = {e0, N8 - 4 - e0, N8 + e0, Nq - 4 - e0, Nq + e0, 3 * N8 - 4 - e0, 3 * N8 + e0, Nh - 4 - e0};
    f32x4 x[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) x[u] = load_row_y4<SRC, WITH_IQ>(SRCP, IP, QP, row, W, u < 8 ? pos[u] : W - 4 - pos[15 - u]);
    // level 1 at the positions of quads 0..7
    f64x4 S[8], D[8];
#pragma unroll
    for (int u = 0; u < 8; ++u)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            S[u][i] = (double)x[u][i] + (double)x[15 - u][3 - i];
            D[u][i] = (double)x[u][i] - (double)x[15 - u][3 - i];
        }
    // D (DCT-IV input of length n/2): the unit at e0 and its mirror unit at n/8 - 4 - e0.  AS and BD (class E: a DCT-II
    // and a DST-II of length n/8) fold once more with their mirrors -- element e0 + i meets element n/8 - 1 - (e0 + i), which
    // is element 3 - i of the mirror unit: exact additions -- into AS+ AS- BD+ BD- of length n/16 (launches E even / odd)
    {
        f64x4 as, bd, ad, bs, asm_, bdm_, adm_, bsm_;
        split_unit(D[0], D[3], D[4], D[7], rot1, e0, Nq, as, bd, ad, bs);
        split_unit(D[1], D[2], D[5], D[6], rot1, N8 - 4 - e0, Nq, asm_, bdm_, adm_, bsm_);
        if (efold) {
            f64x4 p, m, q, r;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                p[i] = as[i] + asm_[3 - i]; m[i] = as[i] - asm_[3 - i];
                q[i] = bd[i] + bdm_[3 - i]; r[i] = bd[i] - bdm_[3 - i];
            }
            put(static_cast<double*>(dp.asp), e0, p); put(static_cast<double*>(dp.asm_), e0, m);
            put(static_cast<double*>(dp.bdp), e0, q); put(static_cast<double*>(dp.bdm), e0, r);
            // Class O: X[8i+5] = T(i) + U(i), X[8i+3] = T(i) - U(i) with T the DCT-IV of AD and U the DST-IV of BS, length
            // L = n/8; U(i) = (-1)^i DCT-IV(reversed BS)(i).  One more rotation of the pairs (n, L-1-n), angle pi (2n+1) / (4L)
            // (the table of a length-n/4 axis), turns a DCT-IV of length L into a DCT-II of a and a DST-II of b, length L/2:
            //   a = d[n] cos + d[L-1-n] sin,  b = d[L-1-n] cos - d[n] sin;   even outputs A[j] + B[j], odd ones A[j] - B[j].
            // With (a, b) of AD plus / minus (a, b) of the reversed BS the two signs of (-1)^i sort themselves into two
            // launches of the class-E shape on the bases of E even: P -> 16j + 5, 16j - 5;  M -> 16j + 3, 16j - 3.
            const f64x4 c3 = *reinterpret_cast<const f64x4*>(rot3 + e0), s3 = *reinterpret_cast<const f64x4*>(rot3 + N16 + e0);
            f64x4 oap, obp, oam, obm;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const double cc = c3[i], ss = s3[i];
                const double au = ad[i] * cc + adm_[3 - i] * ss, bu = adm_[3 - i] * cc - ad[i] * ss;
                const double av = bsm_[3 - i] * cc + bs[i] * ss, bv = bs[i] * cc - bsm_[3 - i] * ss;
                oap[i] = au + av; obp[i] = bu + bv;
                oam[i] = au - av; obm[i] = bu - bv;
            }
            put(static_cast<double*>(dp.oap), e0, oap); put(static_cast<double*>(dp.obp), e0, obp);
            put(static_cast<double*>(dp.oam), e0, oam); put(static_cast<double*>(dp.obm), e0, obm);
        } else {
            put(static_cast<double*>(dp.as), e0, as); put(static_cast<double*>(dp.bd), e0, bd);
            put(static_cast<double*>(dp.as), N8 - 4 - e0, asm_); put(static_cast<double*>(dp.bd), N8 - 4 - e0, bdm_);
            put(AD, e0, ad); put(BS, e0, bs);
            put(AD, N8 - 4 - e0, adm_); put(BS, N8 - 4 - e0, bsm_);
        }
    }
    // level 2 on S (length n/2): quad u mirrors quad 7 - u
    f64x4 SS[4], SD[4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            SS[u][i] = S[u][i] + S[7 - u][3 - i];
            SD[u][i] = S[u][i] - S[7 - u][3 - i];
        }
    // SD (DCT-IV input of length n/4): one unit at e0
    {
        f64x4 as, bd, ad, bs;
        split_unit(SD[0], SD[1], SD[2], SD[3], rot2, e0, N8, as, bd, ad, bs);
        put(AS2, e0, as); put(BD2, e0, bd); put(AD2, e0, ad); put(BS2, e0, bs);
    }
    // level 3 on SS (length n/4): quad 0 mirrors quad 3, quad 1 mirrors quad 2
    f64x4 r1q[2], r2q[2];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            r1q[u][i] = SS[u][i] + SS[3 - u][3 - i];
            r2q[u][i] = SS[u][i] - SS[3 - u][3 - i];
        }
    if (efold) {
        // R1 (a DCT-II input of length n/8) folds with its mirror (exact); R2 (a DCT-IV input) rotates like class O above
        const f64x4 c3 = *reinterpret_cast<const f64x4*>(rot3 + e0), s3 = *reinterpret_cast<const f64x4*>(rot3 + N16 + e0);
        f64x4 p, m, a, b;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            p[i] = r1q[0][i] + r1q[1][3 - i];
            m[i] = r1q[0][i] - r1q[1][3 - i];
            const double cc = c3[i], ss = s3[i];
            a[i] = r2q[0][i] * cc + r2q[1][3 - i] * ss;
            b[i] = r2q[1][3 - i] * cc - r2q[0][i] * ss;
        }
        put(static_cast<double*>(dp.r1p), e0, p); put(static_cast<double*>(dp.r1m), e0, m);
        put(static_cast<double*>(dp.r2a), e0, a); put(static_cast<double*>(dp.r2b), e0, b);
        return;
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        put(R1, pos[u], r1q[u]);
        put(R2, pos[u], r2q[u]);
    }
    if (e0 == 0)
        for (unsigned z = N8; z < K8; z += 4) {
            put(AD, z, zero); put(BS, z, zero); put(R1, z, zero); put(R2, z, zero);
            put(static_cast<double*>(dp.as), z, zero); put(static_cast<double*>(dp.bd), z, zero);
        }
}

// ---------------------------------------------------------------------------------------------
// Three folding levels on a forward COLUMN pass (H % 32 == 0; pays from ~3000 rows: 8K frames): the same
// folds as pair_prep8_rows_kernel, per column, transposed through LDS.  Lines = (frame, column); one block =
// 32 eighth-indices e x 32 columns; per (e, column) the 8 rows that meet in e:
//   rows  e, Hq-1-e, Hq+e, Hh-1-e, Hh+e, 3Hq-1-e, 3Hq+e, H-1-e      (Hq = H/4, Hh = H/2; row u mirrors row 7-u)
//   S[u] = x[u] + x[7-u], P(pos u) = x[u] - x[7-u]   (u < 4: positions e, Hq-1-e, Hq+e, Hh-1-e of the half axis)
//   SS[0] = S[0] + S[3], SS[1] = S[1] + S[2];  M(e) = S[0] - S[3], M(Hq-1-e) = S[1] - S[2]
//   R1(e) = SS[0] + SS[1], R2(e) = SS[0] - SS[1]
// R1, R2: K8 = kpad(H/4) wide; M: Kq = kpad(H/2); P: Kp = kpad(H); k-blocked, zero padded.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pair_prep8_cols_kernel(const float* __restrict__ IN, double* __restrict__ R1,
                                                             double* __restrict__ R2, double* __restrict__ M, double* __restrict__ P,
                                                             unsigned W, unsigned H, unsigned K8, unsigned Kq, unsigned Kp,
                                                             unsigned n_frames, unsigned tiles_e, unsigned tiles_c) {
    __shared__ double s[4][32][33];            // first R1, R2, M(e), M(Hq-1-e); then the four positions of P (34 KB in f64)
    const unsigned Hh = H / 2, Hq = H / 4, He = H / 8;
    const unsigned z = blockIdx.x / (tiles_e * tiles_c);
    const unsigned tt = blockIdx.x % (tiles_e * tiles_c);
    const unsigned e0 = (tt % tiles_e) * 32, c0 = (tt / tiles_e) * 32;
    const float* __restrict__ Pz = IN + (size_t)z * H * W;
    const unsigned tid = threadIdx.x;
    const unsigned er = tid >> 3, cq = (tid & 7) * 4;              // load side: one e, 4 columns
    const unsigned cl = tid & 31, kq = (tid >> 5) * 4;             // store side: one column, 4 consecutive e
    const unsigned cw = c0 + cl, ew = e0 + kq;
    const bool wr = cw < W && ew < K8;
    const size_t line = (size_t)z * W + cw, lines = (size_t)n_frames * W;
    auto fwd = [&](int a) { return (f64x4){s[a][cl][kq], s[a][cl][kq + 1], s[a][cl][kq + 2], s[a][cl][kq + 3]}; };
    auto rev = [&](int a) { return (f64x4){s[a][cl][kq + 3], s[a][cl][kq + 2], s[a][cl][kq + 1], s[a][cl][kq]}; };
    double d1[4][4];                                                     // P values of this thread's (e, 4 columns), kept for the second round
    {
        const unsigned e = e0 + er;
        unsigned c = c0 + cq;
        c = c + 4 <= W ? c : W - 4;                               // W % 4 == 0; duplicates are never written out
        f32x4 x[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) x[u] = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (e < He) {
            const unsigned rows[8] = {e, Hq - 1 - e, Hq + e, Hh - 1 - e, Hh + e, 3 * Hq - 1 - e, 3 * Hq + e, H - 1 - e};
#pragma unroll
            for (int u = 0; u < 8; ++u) x[u] = *reinterpret_cast<const f32x4*>(Pz + (size_t)rows[u] * W + c);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            double S[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                S[u] = (double)x[u][i] + (double)x[7 - u][i];
                d1[u][i] = (double)x[u][i] - (double)x[7 - u][i];
            }
            const double ss0 = S[0] + S[3], ss1 = S[1] + S[2];
            s[0][cq + i][er] = ss0 + ss1;
            s[1][cq + i][er] = ss0 - ss1;
            s[2][cq + i][er] = S[0] - S[3];
            s[3][cq + i][er] = S[1] - S[2];
        }
    }
    __syncthreads();
    if (wr) {
        *reinterpret_cast<f64x4*>(R1 + blk_index<double>(line, ew, lines)) = fwd(0);      // zero beyond He (x was zero)
        *reinterpret_cast<f64x4*>(R2 + blk_index<double>(line, ew, lines)) = fwd(1);
        if (ew < He) {                                              // He % 4 == 0: whole quads
            *reinterpret_cast<f64x4*>(M + blk_index<double>(line, ew, lines)) = fwd(2);
            *reinterpret_cast<f64x4*>(M + blk_index<double>(line, Hq - 4 - ew, lines)) = rev(3);
        }
        if (ew == 0)
            for (unsigned zz = Hq; zz < Kq; zz += 4) *reinterpret_cast<f64x4*>(M + blk_index<double>(line, zz, lines)) = (f64x4){0, 0, 0, 0};
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int i = 0; i < 4; ++i) s[u][cq + i][er] = d1[u][i];
    __syncthreads();
    if (wr) {
        if (ew < He) {
            *reinterpret_cast<f64x4*>(P + blk_index<double>(line, ew, lines)) = fwd(0);
            *reinterpret_cast<f64x4*>(P + blk_index<double>(line, Hq - 4 - ew, lines)) = rev(1);
            *reinterpret_cast<f64x4*>(P + blk_index<double>(line, Hq + ew, lines)) = fwd(2);
            *reinterpret_cast<f64x4*>(P + blk_index<double>(line, Hh - 4 - ew, lines)) = rev(3);
        }
        if (ew == 0)
            for (unsigned zz = Hh; zz < Kp; zz += 4) *reinterpret_cast<f64x4*>(P + blk_index<double>(line, zz, lines)) = (f64x4){0, 0, 0, 0};
    }
}

// ---------------------------------------------------------------------------------------------
// The deep forward pre-pass of a COLUMN pass (H % 16 == 0) over ONE-TILE CLASS-MAJOR input: the row pass wrote the plane
// class-major with the whole line as its one tile, because 128 does not divide W (ForwardClassLayout{W, W}; every other
// plane takes the kernels of dct_pair_prep_staged.hip).  The same planes as pair_prep16_rows_kernel, lines = (frame,
// column), transposed through LDS.  One block = 32 units e < H/16 x 32 memory columns; per (e, column) the 16 rows
// that meet in e (row u mirrors row 15 - u).  Four LDS rounds of four planes each (34 KB):
//   0: AS BD AD BS at e            1: the same planes at the mirror unit H/8 - 1 - e
//   2: AS2 BD2 AD2 BS2 at e        3: R1 R2 at e and at H/8 - 1 - e
// ---------------------------------------------------------------------------------------------
// v[0 .. nvalid) -> plane positions k0 .. (ascending); one 32-byte store when the run is a whole aligned quad
__device__ inline void store_run(double* __restrict__ plane, size_t line, size_t lines, unsigned k0, const double (&v)[4], unsigned nvalid) {
    if (nvalid == 4 && (k0 & 3u) == 0) {
        *reinterpret_cast<f64x4*>(plane + blk_index<double>(line, k0, lines)) = (f64x4){v[0], v[1], v[2], v[3]};
    } else {
        for (unsigned j = 0; j < nvalid; ++j) plane[blk_index<double>(line, k0 + j, lines)] = v[j];
    }
}

// efold: the row pass ran at level 2 (the sixteen-class order of ForwardClassLayout)
__global__ __launch_bounds__(256) void pair_prep16_cols_onetile_kernel(const float* __restrict__ IN, DeepPlanes dp,
                                                                      const double* __restrict__ rot1, const double* __restrict__ rot2,
                                                                      unsigned W, unsigned H, unsigned K8, unsigned K16,
                                                                      unsigned n_frames, unsigned tiles_e, unsigned tiles_c, unsigned efold) {
    __shared__ double s[4][32][33];
    const unsigned Hh = H / 2, Hq = H / 4, H8 = H / 8, H16 = H / 16;      // H16: units
    const unsigned z = blockIdx.x / (tiles_e * tiles_c);
    const unsigned tt = blockIdx.x % (tiles_e * tiles_c);
    const unsigned e0 = (tt % tiles_e) * 32, c0 = (tt / tiles_e) * 32;
    const float* __restrict__ Pz = IN + (size_t)z * H * W;
    const unsigned tid = threadIdx.x;
    const unsigned er = tid >> 3, cq = (tid & 7) * 4;              // load side: one e, 4 columns
    const unsigned cl = tid & 31, kq = (tid >> 5) * 4;             // store side: one column, 4 consecutive e
    const bool col_ok = c0 + cl < W;
    const unsigned cw = c0 + cl, ew = e0 + kq;
    // memory column cw of the intermediate plane holds frequency natural(cw) of the row pass (class-major order): the
    // operand line -- and with it the output column of the column GEMMs -- is the natural one
    const unsigned cn = col_ok ? ForwardClassLayout{W, W, efold != 0}.natural(cw) : cw;
    const size_t line = (size_t)z * W + cn, lines = (size_t)n_frames * W;
    double* planes8[6] = {static_cast<double*>(dp.as), static_cast<double*>(dp.bd), static_cast<double*>(dp.ad), static_cast<double*>(dp.bs),
                     static_cast<double*>(dp.r1), static_cast<double*>(dp.r2)};
    double* planes16[4] = {static_cast<double*>(dp.as2), static_cast<double*>(dp.bd2), static_cast<double*>(dp.ad2), static_cast<double*>(dp.bs2)};
    const unsigned e = e0 + er;
    const bool unit_ok = e < H16;
    const unsigned ec = unit_ok ? e : 0;                           // table indices stay in range
    f32x4 x[16];
    {
        unsigned c = c0 + cq;
        c = c + 4 <= W ? c : W - 4;                               // W % 4 == 0; duplicates are never written out
#pragma unroll
        for (int u = 0; u < 16; ++u) x[u] = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (unit_ok) {
            const unsigned rp[8] = {e, H8 - 1 - e, H8 + e, Hq - 1 - e, Hq + e, 3 * H8 - 1 - e, 3 * H8 + e, Hh - 1 - e};
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                x[u] = *reinterpret_cast<const f32x4*>(Pz + (size_t)rp[u] * W + c);
                x[15 - u] = *reinterpret_cast<const f32x4*>(Pz + (size_t)(H - 1 - rp[u]) * W + c);
            }
        }
    }
    const unsigned nvalid = !col_ok ? 0u : (ew >= H16 ? 0u : (H16 - ew < 4 ? H16 - ew : 4u));      // valid units of the store quad
    auto gather = [&](int a, double (&v)[4], bool reverse) {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = s[a][cl][kq + j];
        if (reverse) {                                              // first nvalid entries, reversed
            double w[4] = {0, 0, 0, 0};
            for (unsigned j = 0; j < nvalid; ++j) w[j] = v[nvalid - 1 - j];
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = w[j];
        }
    };
#pragma unroll 1
    for (int round = 0; round < 4; ++round) {
        if (round) __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            double D[8], S[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                S[u] = (double)x[u][i] + (double)x[15 - u][i];
                D[u] = (double)x[u][i] - (double)x[15 - u][i];
            }
            double o[4] = {0, 0, 0, 0};
            if (round == 0) {
                split_one(D[0], D[3], D[4], D[7], rot1, ec, Hq, o[0], o[1], o[2], o[3]);
            } else if (round == 1) {
                split_one(D[1], D[2], D[5], D[6], rot1, H8 - 1 - ec, Hq, o[0], o[1], o[2], o[3]);
            } else {
                double SS[4], SD[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) { SS[u] = S[u] + S[7 - u]; SD[u] = S[u] - S[7 - u]; }
                if (round == 2) {
                    split_one(SD[0], SD[1], SD[2], SD[3], rot2, ec, H8, o[0], o[1], o[2], o[3]);
                } else {
                    o[0] = SS[0] + SS[3]; o[1] = SS[0] - SS[3];      // R1, R2 at e
                    o[2] = SS[1] + SS[2]; o[3] = SS[1] - SS[2];      // R1, R2 at H/8 - 1 - e
                }
            }
#pragma unroll
            for (int a = 0; a < 4; ++a) s[a][cq + i][er] = unit_ok ? o[a] : 0.0;
        }
        __syncthreads();
        if (col_ok && ew < K16) {
            double v[4];
            if (round == 0) {
#pragma unroll
                for (int a = 0; a < 4; ++a) { gather(a, v, false); store_run(planes8[a], line, lines, ew, v, nvalid); }
            } else if (round == 1) {
#pragma unroll
                for (int a = 0; a < 4; ++a) { gather(a, v, true); if (nvalid) store_run(planes8[a], line, lines, H8 - ew - nvalid, v, nvalid); }
            } else if (round == 2) {
#pragma unroll
                for (int a = 0; a < 4; ++a) { gather(a, v, false); store_run(planes16[a], line, lines, ew, v, 4u); }   // zeros beyond H/16
            } else {
                gather(0, v, false); store_run(planes8[4], line, lines, ew, v, nvalid);
                gather(1, v, false); store_run(planes8[5], line, lines, ew, v, nvalid);
                gather(2, v, true); if (nvalid) store_run(planes8[4], line, lines, H8 - ew - nvalid, v, nvalid);
                gather(3, v, true); if (nvalid) store_run(planes8[5], line, lines, H8 - ew - nvalid, v, nvalid);
                if (ew == 0)
                    for (unsigned k = H8; k < K8; ++k)
#pragma unroll
                        for (int a = 0; a < 6; ++a) planes8[a][blk_index<double>(line, k, lines)] = 0.0;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Launchers
// ---------------------------------------------------------------------------------------------
size_t dct_pair_operand_elems(size_t n_frames, size_t w, size_t h) {
    const size_t a = n_frames * h * pair_kpad(w), b = n_frames * w * pair_kpad(h);
    return a > b ? a : b;
}

int launch_dct_pair_prep(hipStream_t st, bool is_row, bool inverse, const float* in, size_t n_frames, size_t w, size_t h,
                         double* o1, double* o2) {
    if (n_frames == 0) return SSW_OK;
    if (w > 0xFFFFFFull || h > 0xFFFFFFull || n_frames > 0xFFFFFFull) return SSW_ERR_BAD_DIMS;
    if (is_row) {
        const unsigned Kp = (unsigned)pair_kpad(w), tiles_k = (Kp + 31) / 32;
        const size_t rows = n_frames * h;
        const unsigned long long nblk = (unsigned long long)((rows + 31) / 32) * tiles_k;
        if (rows > 0xFFFFFFFFull || nblk > 0x7FFFFFFFull) return SSW_ERR_BAD_DIMS;
        if (inverse) pair_prep_rows_kernel<true><<<(unsigned)nblk, 256, 0, st>>>(in, o1, o2, (unsigned)rows, (unsigned)w, Kp, tiles_k);
        else         pair_prep_rows_kernel<false><<<(unsigned)nblk, 256, 0, st>>>(in, o1, o2, (unsigned)rows, (unsigned)w, Kp, tiles_k);
    } else {
        const unsigned Kp = (unsigned)pair_kpad(h);
        const unsigned tiles_k = (Kp + 31) / 32, tiles_c = (unsigned)((w + 63) / 64);
        const unsigned long long nblk = (unsigned long long)tiles_k * tiles_c * n_frames;
        if (nblk > 0x7FFFFFFFull) return SSW_ERR_BAD_DIMS;
        if (inverse) pair_prep_cols_kernel<true><<<(unsigned)nblk, 256, 0, st>>>(in, o1, o2, (unsigned)w, (unsigned)h, Kp, (unsigned)n_frames, tiles_k, tiles_c);
        else         pair_prep_cols_kernel<false><<<(unsigned)nblk, 256, 0, st>>>(in, o1, o2, (unsigned)w, (unsigned)h, Kp, (unsigned)n_frames, tiles_k, tiles_c);
    }
    SSW_HIP_CHECK(hipGetLastError());
    return SSW_OK;
}

// rows-first forward transform: the row pre-pass reads the plane or the interleaved RGB frames themselves (in.i / in.q, both or
// neither, receive the I and Q planes); column and inverse passes read a plane
int launch_dct_pair_prep4(hipStream_t st, bool is_row, bool inverse, const RowInput& in, size_t n_frames, size_t w, size_t h,
                          double* q1, double* q2, double* p) {
    if (n_frames == 0) return SSW_OK;
    const bool plane = in.kind == RowSrc::Plane;
    if (w > 0xFFFFFFull || h > 0xFFFFFFull || (plane && n_frames > 0xFFFFFFull)) return SSW_ERR_BAD_DIMS;
    if (!plane && (!is_row || inverse)) return SSW_ERR_BAD_ARG;
    const size_t len = is_row ? w : h;
    const unsigned Kp = (unsigned)pair_kpad(len), Kq = (unsigned)pair_kpad(len / 2);
    const unsigned tiles_q = (Kq + 31) / 32;
    const float* x = static_cast<const float*>(in.p);
    if (is_row) {
        const size_t rows = n_frames * h;
        const unsigned long long nblk = (unsigned long long)((rows + 31) / 32) * tiles_q;
        if (rows > 0xFFFFFFFFull || nblk > 0x7FFFFFFFull) return SSW_ERR_BAD_DIMS;
        if (inverse) pair_prep4_rows_kernel<true, RowSrc::Plane, false><<<(unsigned)nblk, 256, 0, st>>>(x, q1, q2, p, nullptr, nullptr, (unsigned)rows, (unsigned)w, Kq, Kp, tiles_q);
        else SSW_TRY(dispatch_row_src(in, [&](auto src, auto iq) {
            pair_prep4_rows_kernel<false, decltype(src)::value, decltype(iq)::value><<<(unsigned)nblk, 256, 0, st>>>(
                in.p, q1, q2, p, in.i, in.q, (unsigned)rows, (unsigned)w, Kq, Kp, tiles_q);
        }));
    } else {
        const unsigned tiles_c = (unsigned)((w + 31) / 32);
        const unsigned long long nblk = (unsigned long long)tiles_q * tiles_c * n_frames;
        if (nblk > 0x7FFFFFFFull) return SSW_ERR_BAD_DIMS;
        if (inverse) pair_prep4_cols_kernel<true><<<(unsigned)nblk, 256, 0, st>>>(x, q1, q2, p, (unsigned)w, (unsigned)h, Kq, Kp, (unsigned)n_frames, tiles_q, tiles_c);
        else         pair_prep4_cols_kernel<false><<<(unsigned)nblk, 256, 0, st>>>(x, q1, q2, p, (unsigned)w, (unsigned)h, Kq, Kp, (unsigned)n_frames, tiles_q, tiles_c);
    }
    SSW_HIP_CHECK(hipGetLastError());
    return SSW_OK;
}

// third folding level along the rows (forward row passes only)
int launch_dct_pair_prep8_rows(hipStream_t st, const RowInput& in, size_t n_frames, size_t w, size_t h,
                               double* r1, double* r2, double* m, double* p) {
    if (n_frames == 0) return SSW_OK;
    if (w > 0xFFFFFFull || h > 0xFFFFFFull) return SSW_ERR_BAD_DIMS;
    const unsigned Kp = (unsigned)pair_kpad(w), Kq = (unsigned)pair_kpad(w / 2), K8 = (unsigned)pair_kpad(w / 4);
    const unsigned tiles_e = (K8 + 31) / 32;
    const size_t rows = n_frames * h;
    const unsigned long long nblk = (unsigned long long)((rows + 31) / 32) * tiles_e;
    if (rows > 0xFFFFFFFFull || nblk > 0x7FFFFFFFull) return SSW_ERR_BAD_DIMS;
    SSW_TRY(dispatch_row_src(in, [&](auto src, auto iq) {
        pair_prep8_rows_kernel<decltype(src)::value, decltype(iq)::value><<<(unsigned)nblk, 256, 0, st>>>(
            in.p, r1, r2, m, p, in.i, in.q, (unsigned)rows, (unsigned)w, K8, Kq, Kp, tiles_e);
    }));
    SSW_HIP_CHECK(hipGetLastError());
    return SSW_OK;
}

// three levels on a forward column pass (H % 32 == 0): (SSS, SS-) [kpad(h/4) wide], S- [kpad(h/2)], x- [kpad(h)]
int launch_dct_pair_prep8_cols(hipStream_t st, const float* in, size_t n_frames, size_t w, size_t h,
                               double* r1, double* r2, double* m, double* p) {
    if (n_frames == 0) return SSW_OK;
    if (w > 0xFFFFFFull || h > 0xFFFFFFull || n_frames > 0xFFFFFFull) return SSW_ERR_BAD_DIMS;
    const unsigned Kp = (unsigned)pair_kpad(h), Kq = (unsigned)pair_kpad(h / 2), K8 = (unsigned)pair_kpad(h / 4);
    const unsigned tiles_e = (K8 + 31) / 32, tiles_c = (unsigned)((w + 31) / 32);
    const unsigned long long nblk = (unsigned long long)tiles_e * tiles_c * n_frames;
    if (nblk > 0x7FFFFFFFull) return SSW_ERR_BAD_DIMS;
    pair_prep8_cols_kernel<<<(unsigned)nblk, 256, 0, st>>>(in, r1, r2, m, p, (unsigned)w, (unsigned)h, K8, Kq, Kp, (unsigned)n_frames, tiles_e, tiles_c);
    SSW_HIP_CHECK(hipGetLastError());
    return SSW_OK;
}

// deep forward row pre-pass of any RowInput;
// base: 6 planes of lines * K8 doubles (AS BD AD BS R1 R2) followed by 4 planes of lines * K16 (AS2 BD2 AD2 BS2)
// 6 planes K8 wide + 4 K16 wide, or (forward row passes at level 2) 16 planes K16 wide
size_t dct_pair_deep_elems(size_t lines, size_t len) {
    const size_t k8 = dct_pair_split_kpad(len), k16 = dct_pair_split_kpad(len / 2);
    return lines * (6 * k8 + 4 * k16 > 16 * k16 ? 6 * k8 + 4 * k16 : 16 * k16);
}
int launch_dct_pair_prep16_rows(hipStream_t st, const RowInput& in, size_t n_frames, size_t w, size_t h, double* base,
                                const double* rot1, const double* rot2, const double* rot3, bool l2, bool unit_order) {
    if (n_frames == 0) return SSW_OK;
    if (w > 0xFFFFFFull || h > 0xFFFFFFull || w % 64 != 0) return SSW_ERR_BAD_DIMS;
    const unsigned K8 = (unsigned)dct_pair_split_kpad(w), K16 = (unsigned)dct_pair_split_kpad(w / 2);
    const unsigned tiles_e = (K16 + 31) / 32;
    if (unit_order && (h % 16 != 0 || !l2)) return SSW_ERR_BAD_ARG;
    const unsigned unit_hup = unit_order ? (unsigned)dct_pair_fused_units(h) : 0u;
    const size_t rows = unit_order ? n_frames * 16 * unit_hup : n_frames * h;       // operand lines
    const unsigned long long nblk = (unsigned long long)((rows + 31) / 32) * tiles_e;
    if (rows > 0xFFFFFFFFull || nblk > 0x7FFFFFFFull) return SSW_ERR_BAD_DIMS;
    DeepPlanes dp = planes_of(base, rows, K8, K16);
    const unsigned efold = l2 ? 1u : 0u;
    if (efold) {     // level 2: sixteen planes K16 wide, in this order (build_pass and the pruned pass index them by number)
        void** const pl[16] = {&dp.asp, &dp.asm_, &dp.bdp, &dp.bdm, &dp.oap, &dp.obp, &dp.oam, &dp.obm,
                               &dp.r1p, &dp.r1m, &dp.r2a, &dp.r2b, &dp.as2, &dp.bd2, &dp.ad2, &dp.bs2};
        for (int j = 0; j < 16; ++j) *pl[j] = base + (size_t)j * rows * K16;
        dp.as = dp.bd = dp.ad = dp.bs = dp.r1 = dp.r2 = nullptr;
        if (!rot3) return SSW_ERR_BAD_ARG;
    }
    if (efold && dct_pair_prep_light_ok(w, rows))          // r5: the form that runs beside the GEMMs of the other lane (dct_pair_prep_light.hip)
        return launch_dct_pair_prep16_rows_light(st, in, dp, rot1, rot2, rot3, rows, w, K16, unit_order ? (unsigned)h : 0u, unit_hup);
    SSW_TRY(dispatch_row_src(in, [&](auto src, auto iq) {
        pair_prep16_rows_kernel<decltype(src)::value, decltype(iq)::value><<<(unsigned)nblk, 256, 0, st>>>(
            in.p, dp, rot1, rot2, rot3, in.i, in.q, (unsigned)rows, (unsigned)w, K8, K16, tiles_e, efold, unit_order ? (unsigned)h : 0u, unit_hup);
    }));
    SSW_HIP_CHECK(hipGetLastError());
    return SSW_OK;
}

// deep forward column pre-pass (H % 16 == 0): same plane order as the row version, lines = n_frames * w;
// semi-deep: H % 8 == 0 but not % 16 (1080 rows): D split, SS folded a third time, SD left whole
size_t dct_pair_semi_deep_elems(size_t lines, size_t len) { return lines * (6 * dct_pair_split_kpad(len) + pair_kpad(len / 2)); }
int launch_dct_pair_prep16_cols(hipStream_t st, const float* in, size_t n_frames, size_t w, size_t h, double* base,
                                const double* rot1, const double* rot2, const double* rot3, PrepFamily prep, const PairLayout& lay) {
    if (n_frames == 0) return SSW_OK;
    const bool semi = h % 16 != 0, class_major = lay.class_major;
    if (w > 0xFFFFFFull || h > 0xFFFFFFull || n_frames > 0xFFFFFFull || h % 8 != 0 || w % 4 != 0) return SSW_ERR_BAD_DIMS;
    const unsigned K8 = (unsigned)dct_pair_split_kpad(h);
    const unsigned K16 = semi ? (unsigned)pair_kpad(h / 2) : (unsigned)dct_pair_split_kpad(h / 2);      // semi: width of the SD plane
    if (prep == PrepFamily::L2)
        return launch_prep16_cols_l2(st, in, n_frames, w, h, base, rot1, rot2, rot3, class_major, class_major && lay.rows_l2, K16);
    if (prep == PrepFamily::Staged)
        return launch_prep16_cols_staged(st, in, n_frames, w, h, base, rot1, rot2, class_major, semi, K8, K16, lay.rows_l2);
    // PrepFamily::OneTile: deep columns of a class-major plane whose one tile is the whole line (dct_plan.hip: col_prep)
    if (semi || !class_major || lay.tile != w) return SSW_ERR_BAD_ARG;
    const unsigned tiles_e = (K16 + 31) / 32, tiles_c = (unsigned)((w + 31) / 32);
    const unsigned long long nblk = (unsigned long long)tiles_e * tiles_c * n_frames;
    if (nblk > 0x7FFFFFFFull) return SSW_ERR_BAD_DIMS;
    pair_prep16_cols_onetile_kernel<<<(unsigned)nblk, 256, 0, st>>>(in, planes_of(base, n_frames * w, K8, K16), rot1, rot2, (unsigned)w, (unsigned)h, K8, K16,
                                                                      (unsigned)n_frames, tiles_e, tiles_c, lay.rows_l2 ? 1u : 0u);
    SSW_HIP_CHECK(hipGetLastError());
    return SSW_OK;
}

}  // namespace ssw
