// Fingerprinting: many individually marked copies of ONE image per call -- Writer::new(image, cfg).mark(&[&mark_i])
// (src/algorithm.rs:295-316, :355-379) for every recipient i, the loop of examples/main.rs:266-278 once per mark.
//
// Every copy shares the forward transform, the coefficient plane C and the index list; copies differ only in the k
// coefficients Delta_i = c'_i - c_i.  The inverse (src/dct2d.rs:83-219, larger dimension first) is two 1-D passes with an
// f32 store between them, so a changed coefficient changes the intermediate plane only in the first-pass lines that hold
// it (R of them: 46 at 4K for k = 1000).  With A the first-pass axis (rows when w >= h) and B the second:
//   base, once per image     T32  = first pass of C, rounded to f32 (the dense f64 GEMM of dct.hip)
//                            T64  = the same first pass unrounded, for the R lines only (T32 takes round(T64) there)
//                            Yr64 = second pass of T32, kept in f64 (dct.hip, f64-store variant)
//   per copy n               T'[r][:] = round_f32(T64[r][:] + sum_{i on line r} Delta_i b_A(v_i, :)),  dT = T' - T32 (exact)
//                            Y'  = Yr64 + sum_{r in R} b_B(r, .) dT[r][.]        (v_mfma_f64_16x16x4_f64, K = R from device memory)
//                            then the inverse epilogue: round to f32, x 4/(W H), YIQ -> RGB with the original I / Q, clamp
//                            (8-bit: round(c * 255)).
// In exact arithmetic Y' is the second pass of the reference's own intermediate plane for copy n; what remains is f64
// noise of the kind the folded GEMMs carry.  Every copy runs the same operations in the same order whatever the group
// it shares a launch with, so a copy is bit-identical alone or at any position among others.
//
// The inverse basis is read off the cached forward one: E[a][v] = v == 0 ? 1/4 : cos(pi v (2a + 1) / 2N) / 2 =
// D[v][a] / 4 (exact: both come from the same f64 cospi), so the basis "column" v of the inverse is the contiguous row v
// of the forward basis.
#include "dct_pair_common.hpp"
#include "embed_fn.hpp"
#include "ssw_host.hpp"

#include <algorithm>

namespace ssw {

namespace {

constexpr unsigned FP_KSTEP = 16;          // R is padded to whole groups of four MFMA k-steps (zero rows in both operands)
constexpr unsigned FP_SLOT_BLOCKS = 32;    // grid extent over slots: blocks stride over the R slots read from device memory
constexpr unsigned FP_SCAN_THREADS = 1024;

// line / position of a flat coefficient index along the first pass
__device__ inline unsigned fp_line(uint32_t idx, unsigned w, bool rows_first) { return rows_first ? idx / w : idx % w; }
__device__ inline unsigned fp_pos(uint32_t idx, unsigned w, bool rows_first) { return rows_first ? idx % w : idx / w; }
// E[a][v] of the inverse basis of length n from the forward basis fwd (row stride kp)
__device__ inline double fp_inv_basis(const double* __restrict__ fwd, size_t kp, unsigned v, unsigned a) {
    return v == 0 ? 0.25 : 0.25 * fwd[(size_t)v * kp + a];
}

// exclusive scan of one value per thread across a block of FP_SCAN_THREADS threads; *total: the sum
__device__ inline unsigned fp_block_scan(unsigned v, unsigned* total) {
    __shared__ unsigned s[FP_SCAN_THREADS];
    const unsigned t = threadIdx.x;
    s[t] = v;
    __syncthreads();
    for (unsigned d = 1; d < FP_SCAN_THREADS; d <<= 1) {
        const unsigned add = t >= d ? s[t - d] : 0u;
        __syncthreads();
        s[t] += add;
        __syncthreads();
    }
    const unsigned incl = s[t];
    *total = s[FP_SCAN_THREADS - 1];
    __syncthreads();
    return incl - v;
}

// ---- the line plan: distinct first-pass lines of the index list, slot of each, index positions per slot ----------------
__global__ void fp_flag_lines_kernel(const uint32_t* __restrict__ idx, size_t k, unsigned w, bool rows_first, uint32_t* flag) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < k; i += (size_t)gridDim.x * blockDim.x)
        flag[fp_line(idx[i], w, rows_first)] = 1u;
}
// one block: slot_of_line (in place over the flags; ~0u for untouched lines), line_of_slot, info = {R, R padded}
__global__ __launch_bounds__(FP_SCAN_THREADS) void fp_assign_slots_kernel(uint32_t* slot_of_line, uint32_t* line_of_slot,
                                                                          unsigned n_lines, uint32_t* info) {
    const unsigned per = (n_lines + FP_SCAN_THREADS - 1) / FP_SCAN_THREADS;
    const unsigned l0 = threadIdx.x * per, l1 = min(n_lines, l0 + per);
    unsigned cnt = 0;
    for (unsigned l = l0; l < l1; ++l) cnt += slot_of_line[l] != 0u;
    unsigned total;
    unsigned s = fp_block_scan(cnt, &total);
    for (unsigned l = l0; l < l1; ++l) {
        if (slot_of_line[l] != 0u) {
            line_of_slot[s] = l;
            slot_of_line[l] = s++;
        } else {
            slot_of_line[l] = ~0u;
        }
    }
    if (threadIdx.x == 0) {
        info[0] = total;
        info[1] = (total + FP_KSTEP - 1) / FP_KSTEP * FP_KSTEP;
    }
}
__global__ void fp_count_kernel(const uint32_t* __restrict__ idx, size_t k, unsigned w, bool rows_first,
                                const uint32_t* __restrict__ slot_of_line, uint32_t* cnt) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < k; i += (size_t)gridDim.x * blockDim.x)
        atomicAdd(&cnt[slot_of_line[fp_line(idx[i], w, rows_first)]], 1u);
}
// one block: off[s] = first list entry of slot s (off[R] = k), cursor = off
__global__ __launch_bounds__(FP_SCAN_THREADS) void fp_offsets_kernel(const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ info,
                                                                     uint32_t* off, uint32_t* cursor) {
    const unsigned R = info[0];
    const unsigned per = (R + FP_SCAN_THREADS - 1) / FP_SCAN_THREADS;
    const unsigned s0 = threadIdx.x * per, s1 = min(R, s0 + per);
    unsigned c = 0;
    for (unsigned s = s0; s < s1; ++s) c += cnt[s];
    unsigned total;
    unsigned o = fp_block_scan(c, &total);
    for (unsigned s = s0; s < s1; ++s) {
        off[s] = o; cursor[s] = o;
        o += cnt[s];
    }
    if (threadIdx.x == 0) off[R] = total;
}
__global__ void fp_fill_kernel(const uint32_t* __restrict__ idx, size_t k, unsigned w, bool rows_first,
                               const uint32_t* __restrict__ slot_of_line, uint32_t* cursor, uint32_t* list) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < k; i += (size_t)gridDim.x * blockDim.x) {
        const unsigned p = atomicAdd(&cursor[slot_of_line[fp_line(idx[i], w, rows_first)]], 1u);
        list[p] = (uint32_t)i;
    }
}
// each slot's positions in rank order: a fixed summation order per line, independent of the atomics' order
__global__ void fp_sort_lists_kernel(const uint32_t* __restrict__ info, const uint32_t* __restrict__ off, uint32_t* list) {
    const unsigned R = info[0];
    for (unsigned s = blockIdx.x * blockDim.x + threadIdx.x; s < R; s += gridDim.x * blockDim.x) {
        const unsigned a = off[s], b = off[s + 1];
        for (unsigned x = a + 1; x < b; ++x) {
            const uint32_t v = list[x];
            unsigned y = x;
            while (y > a && list[y - 1] > v) { list[y] = list[y - 1]; --y; }
            list[y] = v;
        }
    }
}

// ---- base: T64 of the R lines (and T32 there := round(T64)), the gathered second-pass basis ---------------------------------
__global__ __launch_bounds__(256) void fp_t64_kernel(const float* __restrict__ coef, unsigned w, bool rows_first, unsigned la,
                                                     const double* __restrict__ fwd_a, size_t kp_a,
                                                     const uint32_t* __restrict__ info, const uint32_t* __restrict__ line_of_slot,
                                                     double* __restrict__ t64, float* __restrict__ t32) {
    const unsigned R = info[0];
    const unsigned a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= la) return;
    for (unsigned s = blockIdx.y; s < R; s += gridDim.y) {
        const unsigned r = line_of_slot[s];
        const float* line = rows_first ? coef + (size_t)r * w : coef + r;
        const size_t stride = rows_first ? 1 : w;
        double acc = 0.25 * (double)line[0];
        for (unsigned v = 1; v < la; ++v) acc = fma((double)line[(size_t)v * stride], 0.25 * fwd_a[(size_t)v * kp_a + a], acc);
        t64[(size_t)s * la + a] = acc;
        t32[rows_first ? (size_t)r * w + a : (size_t)a * w + r] = (float)acc;
    }
}
// G[s][b] = E_B[b][line s] for s < R, zero rows up to R padded
__global__ __launch_bounds__(256) void fp_gather_basis_kernel(const double* __restrict__ fwd_b, size_t kp_b, unsigned lb,
                                                              const uint32_t* __restrict__ info,
                                                              const uint32_t* __restrict__ line_of_slot, double* __restrict__ g) {
    const unsigned R = info[0], Rp = info[1];
    const unsigned b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= lb) return;
    for (unsigned s = blockIdx.y; s < Rp; s += gridDim.y)
        g[(size_t)s * lb + b] = s < R ? fp_inv_basis(fwd_b, kp_b, line_of_slot[s], b) : 0.0;
}

// ---- per copy: the coefficient changes, then the changed lines of the intermediate plane ----------------------------------------
// d[n][i] = (f64) c'_i - (f64) c_i with c'_i what embed_kernel writes for a single mark (the same insert_fn)
__global__ __launch_bounds__(256) void fp_mark_delta_kernel(const float* __restrict__ coef, const uint32_t* __restrict__ idx, size_t k_eff,
                                                            const float* __restrict__ marks, size_t mark_stride, int method, float alpha,
                                                            double* __restrict__ d) {
    const size_t n = blockIdx.y;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < k_eff; i += (size_t)gridDim.x * blockDim.x) {
        const float c = coef[idx[i]];
        const float cn = insert_fn(method, alpha, c, marks[n * mark_stride + i]);
        d[n * k_eff + i] = (double)cn - (double)c;
    }
}
// dT[n][s][a] = round_f32(T64[s][a] + sum_i d_i E_A[a][v_i]) - T32 (exact in f64); zero rows from R up to R padded
__global__ __launch_bounds__(256) void fp_line_delta_kernel(const uint32_t* __restrict__ idx, size_t k_eff, unsigned w, bool rows_first,
                                                            unsigned la, const double* __restrict__ fwd_a, size_t kp_a,
                                                            const uint32_t* __restrict__ info, const uint32_t* __restrict__ line_of_slot,
                                                            const uint32_t* __restrict__ off, const uint32_t* __restrict__ list,
                                                            const double* __restrict__ t64, const float* __restrict__ t32,
                                                            const double* __restrict__ d, double* __restrict__ dt, size_t dt_copy_stride) {
    const unsigned R = info[0], Rp = info[1];
    const unsigned a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= la) return;
    const size_t n = blockIdx.z;
    const double* __restrict__ dn = d + n * k_eff;
    double* __restrict__ out = dt + n * dt_copy_stride;
    for (unsigned s = blockIdx.y; s < Rp; s += gridDim.y) {
        if (s >= R) { out[(size_t)s * la + a] = 0.0; continue; }
        const unsigned r = line_of_slot[s];
        double sum = 0.0;
        for (unsigned j = off[s], e = off[s + 1]; j < e; ++j) {
            const uint32_t i = list[j];
            sum = fma(dn[i], fp_inv_basis(fwd_a, kp_a, fp_pos(idx[i], w, rows_first), a), sum);
        }
        const float tn = (float)(t64[(size_t)s * la + a] + sum);
        out[(size_t)s * la + a] = (double)tn - (double)t32[rows_first ? (size_t)r * w + a : (size_t)a * w + r];
    }
}

// ---- the update GEMM with the inverse epilogue --------------------------------------------------------------------------
// out[n][i][j] = rgb(f32(Yr64[i][j] + sum_k P_n[k][i] Q_n[k][j]) * scale, I, Q), k < R padded (info[1]).  P / Q are [Rp][h] /
// [Rp][w] f64; one of them is the copy's dT, the other the gathered basis (copy stride 0).  v_mfma_f64_16x16x4_f64: lane l
// supplies A[i = l & 15][k = l >> 4] = P[k][i] and B[k = l >> 4][j = l & 15] = Q[k][j]; D: col = l & 15, row = (l >> 4) + 4 r.
// Block: 4 waves as 2 x 2, each a 32 x 32 pixel tile (2 x 2 MFMA tiles); Yr64, I and Q of the tile stay in registers while
// the block walks the group's copies, so they are read once per tile.
constexpr unsigned FP_TILE = 64;
template <bool U8>
__global__ __launch_bounds__(256) void fp_update_kernel(const double* __restrict__ yr, const float* __restrict__ ip, const float* __restrict__ qp,
                                                        const double* __restrict__ P, size_t p_stride, const double* __restrict__ Q, size_t q_stride,
                                                        const uint32_t* __restrict__ info, unsigned n_copies, unsigned w, unsigned h,
                                                        float scale, void* __restrict__ out) {
    const unsigned tiles_n = (w + FP_TILE - 1) / FP_TILE;
    const unsigned i0 = (blockIdx.x / tiles_n) * FP_TILE, j0 = (blockIdx.x % tiles_n) * FP_TILE;
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned wi = i0 + (wave >> 1) * 32, wj = j0 + (wave & 1) * 32;
    const unsigned li = lane & 15, lq = lane >> 4;
    const unsigned Rp = info[1];
    const size_t plane = (size_t)w * h;

    double y0[2][2][4];
    float iv[2][2][4], qv[2][2][4];
#pragma unroll
    for (int ti = 0; ti < 2; ++ti)
#pragma unroll
        for (int tj = 0; tj < 2; ++tj)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const unsigned i = wi + 16 * ti + lq + 4 * r, j = wj + 16 * tj + li;
                const bool ok = i < h && j < w;
                const size_t p = (size_t)i * w + j;
                y0[ti][tj][r] = ok ? yr[p] : 0.0;
                iv[ti][tj][r] = ok ? ip[p] : 0.0f;
                qv[ti][tj][r] = ok ? qp[p] : 0.0f;
            }
    // operand columns of this lane (clamped: an edge lane's products land in outputs that are never stored)
    unsigned ai[2], bj[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        ai[t] = min(wi + 16 * t + li, h - 1);
        bj[t] = min(wj + 16 * t + li, w - 1);
    }

    for (unsigned n = 0; n < n_copies; ++n) {
        const double* __restrict__ Pn = P + n * p_stride;
        const double* __restrict__ Qn = Q + n * q_stride;
        f64x4 acc[2][2];
#pragma unroll
        for (int ti = 0; ti < 2; ++ti)
#pragma unroll
            for (int tj = 0; tj < 2; ++tj) acc[ti][tj] = (f64x4){y0[ti][tj][0], y0[ti][tj][1], y0[ti][tj][2], y0[ti][tj][3]};
        for (unsigned k0 = 0; k0 < Rp; k0 += FP_KSTEP) {
            double a[4][2], b[4][2];
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const size_t kk = k0 + 4 * s + lq;
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    a[s][t] = Pn[kk * h + ai[t]];
                    b[s][t] = Qn[kk * w + bj[t]];
                }
            }
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int ti = 0; ti < 2; ++ti)
#pragma unroll
                    for (int tj = 0; tj < 2; ++tj)
                        acc[ti][tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s][ti], b[s][tj], acc[ti][tj], 0, 0, 0);
        }
        // the inverse epilogue: f32 store of the second pass, x 4/(W H) (src/dct2d.rs:213-217), yiq.rs:187-197 (+ into_rgb8)
#pragma unroll
        for (int ti = 0; ti < 2; ++ti)
#pragma unroll
            for (int tj = 0; tj < 2; ++tj)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const unsigned i = wi + 16 * ti + lq + 4 * r, j = wj + 16 * tj + li;
                    if (i >= h || j >= w) continue;
                    const float y = (float)acc[ti][tj][r] * scale;
                    const float iq = iv[ti][tj][r], qq = qv[ti][tj][r];
                    const float c0 = pair_clamp01_med3(1.0f * y + 0.948262f * iq + 0.624013f * qq);
                    const float c1 = pair_clamp01_med3(1.0f * y + -0.276066f * iq + -0.639810f * qq);
                    const float c2 = pair_clamp01_med3(1.0f * y + -1.105450f * iq + 1.729860f * qq);
                    const size_t p = (size_t)n * plane + (size_t)i * w + j;
                    if (U8) {
                        uint8_t* o = static_cast<uint8_t*>(out) + 3 * p;
                        o[0] = (uint8_t)pair_round255(c0);
                        o[1] = (uint8_t)pair_round255(c1);
                        o[2] = (uint8_t)pair_round255(c2);
                    } else {
                        float* o = static_cast<float*>(out) + 3 * p;
                        o[0] = c0; o[1] = c1; o[2] = c2;
                    }
                }
    }
}

unsigned grid_over(size_t items, unsigned per_block, size_t cap = 65535) {
    return (unsigned)std::max<size_t>(1, std::min<size_t>((items + per_block - 1) / per_block, cap));
}

}  // namespace

namespace host {

// Copies of one image: coef = C (the writer's plane as it stands), idx its first k_eff indices, iq_i / iq_q the image's I / Q;
// marks [n_copies][mark_stride] (the first k_eff of each used); out [n_copies][h][w][3] f32 or u8.  t32: an f32 plane of
// scratch.  Enqueues on the context's stream only.
int fingerprint_copies(ssw_ctx* ctx, const ssw_config& c, const float* coef, const uint32_t* idx, size_t k_eff, const float* iq_i,
                       const float* iq_q, size_t w, size_t h, const float* marks, size_t mark_stride, size_t n_copies, void* out,
                       bool u8_out, float* t32) {
    if (n_copies == 0) return SSW_OK;
    if (w > 0xFFFFFFull || h > 0xFFFFFFull) return SSW_ERR_BAD_DIMS;
    hipStream_t st = ctx->stream;
    const bool rows_first = w >= h;                              // src/dct2d.rs:93-98
    const size_t la = rows_first ? w : h, lb = rows_first ? h : w;
    const size_t plane = w * h;
    const size_t out_px = u8_out ? 3 : 3 * sizeof(float);
    // k_eff == 0: R = 0, every copy is Writer::result of the unmarked plane (Yr64 alone)
    const size_t s_max = std::max<size_t>(1, std::min(k_eff, lb));
    const size_t s_pad = (s_max + FP_KSTEP - 1) / FP_KSTEP * FP_KSTEP;
    // workspace of a group: its mark deltas and dT planes; groups keep it near 2 GiB
    const size_t per_copy = s_pad * la * sizeof(double) + std::max<size_t>(k_eff, 1) * sizeof(double);
    const size_t group = std::max<size_t>(1, std::min<size_t>({n_copies, 64, ((size_t)2 << 30) / per_copy}));

    // u32 plan: slot_of_line [lb] | line_of_slot [lb] | cnt [lb] | off [lb + 1] | cursor [lb] | list [k_eff] | info [4]
    const size_t u32_words = 5 * lb + 1 + k_eff + 4;
    SSW_TRY(grow(ctx->fingerprint.line_plan, u32_words * sizeof(uint32_t)));
    SSW_TRY(grow(ctx->fingerprint.t64, (s_pad * la + s_pad * lb) * sizeof(double)));
    SSW_TRY(grow(ctx->fingerprint.yr64, plane * sizeof(double)));
    SSW_TRY(grow(ctx->fingerprint.deltas, group * std::max<size_t>(k_eff, 1) * sizeof(double)));
    SSW_TRY(grow(ctx->fingerprint.dt, group * s_pad * la * sizeof(double)));
    uint32_t* slot_of_line = ctx->fingerprint.line_plan.as<uint32_t>();
    uint32_t* line_of_slot = slot_of_line + lb;
    uint32_t* cnt = line_of_slot + lb;
    uint32_t* off = cnt + lb;
    uint32_t* cursor = off + lb + 1;
    uint32_t* list = cursor + lb;
    uint32_t* info = list + k_eff;
    double* t64 = ctx->fingerprint.t64.as<double>();
    double* g = t64 + s_pad * la;
    double* yr = ctx->fingerprint.yr64.as<double>();
    double* d = ctx->fingerprint.deltas.as<double>();
    double* dt = ctx->fingerprint.dt.as<double>();

    const void *inv_w, *inv_h, *fwd_a, *fwd_b;
    SSW_TRY(get_basis(ctx, w, true, true, BasisKind::Dense, &inv_w));
    SSW_TRY(get_basis(ctx, h, true, true, BasisKind::Dense, &inv_h));
    SSW_TRY(get_basis(ctx, la, false, true, BasisKind::Dense, &fwd_a));
    SSW_TRY(get_basis(ctx, lb, false, true, BasisKind::Dense, &fwd_b));
    const size_t kp_a = dense_basis_kpad(la), kp_b = dense_basis_kpad(lb);
    const unsigned W = (unsigned)w;
    {
        // the line plan and the base: T32, T64 of the R lines (T32 := round(T64) there), Yr64, the gathered basis
        StageTimer t(ctx, SSW_STAGE_EMBED, st);
        SSW_HIP_CHECK(hipMemsetAsync(slot_of_line, 0, 3 * lb * sizeof(uint32_t), st));     // flags, (line_of_slot), counts
        SSW_HIP_CHECK(hipMemsetAsync(info, 0, 4 * sizeof(uint32_t), st));
        if (k_eff) {
            fp_flag_lines_kernel<<<grid_over(k_eff, 256, 4096), 256, 0, st>>>(idx, k_eff, W, rows_first, slot_of_line);
            fp_assign_slots_kernel<<<1, FP_SCAN_THREADS, 0, st>>>(slot_of_line, line_of_slot, (unsigned)lb, info);
            fp_count_kernel<<<grid_over(k_eff, 256, 4096), 256, 0, st>>>(idx, k_eff, W, rows_first, slot_of_line, cnt);
            fp_offsets_kernel<<<1, FP_SCAN_THREADS, 0, st>>>(cnt, info, off, cursor);
            fp_fill_kernel<<<grid_over(k_eff, 256, 4096), 256, 0, st>>>(idx, k_eff, W, rows_first, slot_of_line, cursor, list);
            fp_sort_lists_kernel<<<grid_over(s_max, 64, 1024), 64, 0, st>>>(info, off, list);
            SSW_HIP_CHECK(hipGetLastError());
        }
        if (rows_first) SSW_TRY(launch_dct_rows(st, SSW_PRECISION_F64, coef, t32, h, w, inv_w, Epilogue{1.f, 1.f}));
        else            SSW_TRY(launch_dct_cols(st, SSW_PRECISION_F64, coef, t32, 1, w, h, inv_h, Epilogue{1.f, 1.f}));
        const unsigned sb = (unsigned)std::min<size_t>(s_pad, FP_SLOT_BLOCKS);
        fp_t64_kernel<<<dim3(grid_over(la, 256), sb), 256, 0, st>>>(coef, W, rows_first, (unsigned)la, (const double*)fwd_a, kp_a, info,
                                                                    line_of_slot, t64, t32);
        fp_gather_basis_kernel<<<dim3(grid_over(lb, 256), sb), 256, 0, st>>>((const double*)fwd_b, kp_b, (unsigned)lb, info, line_of_slot, g);
        SSW_HIP_CHECK(hipGetLastError());
        if (rows_first) SSW_TRY(launch_dct_cols_f64out(st, t32, yr, 1, w, h, (const double*)inv_h));
        else            SSW_TRY(launch_dct_rows_f64out(st, t32, yr, h, w, (const double*)inv_w));
    }
    const float scale = (float)4 / (float)(w * h);                                          // src/dct2d.rs:213-217
    const unsigned tiles = (unsigned)(((h + FP_TILE - 1) / FP_TILE) * ((w + FP_TILE - 1) / FP_TILE));
    for (size_t n0 = 0; n0 < n_copies; n0 += group) {
        const size_t gn = std::min(group, n_copies - n0);
        {
            StageTimer t(ctx, SSW_STAGE_EMBED, st);
            if (k_eff) {
                fp_mark_delta_kernel<<<dim3(grid_over(k_eff, 256, 1024), (unsigned)gn), 256, 0, st>>>(
                    coef, idx, k_eff, marks + n0 * mark_stride, mark_stride, c.method, c.alpha, d);
                fp_line_delta_kernel<<<dim3(grid_over(la, 256), (unsigned)std::min<size_t>(s_pad, FP_SLOT_BLOCKS), (unsigned)gn), 256, 0, st>>>(
                    idx, k_eff, W, rows_first, (unsigned)la, (const double*)fwd_a, kp_a, info, line_of_slot, off, list, t64, t32, d, dt,
                    s_pad * la);
                SSW_HIP_CHECK(hipGetLastError());
            }
        }
        StageTimer t(ctx, SSW_STAGE_YIQ_TO_RGB, st);
        // rows first: P = gathered basis of the columns (i = image row), Q = dT (j = image column); columns first the other way
        const double* P = rows_first ? g : dt;
        const double* Q = rows_first ? dt : g;
        const size_t ps = rows_first ? 0 : s_pad * la, qs = rows_first ? s_pad * la : 0;
        void* o = static_cast<char*>(out) + n0 * plane * out_px;
        if (u8_out) fp_update_kernel<true><<<tiles, 256, 0, st>>>(yr, iq_i, iq_q, P, ps, Q, qs, info, (unsigned)gn, W, (unsigned)h, scale, o);
        else        fp_update_kernel<false><<<tiles, 256, 0, st>>>(yr, iq_i, iq_q, P, ps, Q, qs, info, (unsigned)gn, W, (unsigned)h, scale, o);
        SSW_HIP_CHECK(hipGetLastError());
    }
    return SSW_OK;
}

// ssw_fingerprint_embed(_rgb8): Writer::new on the device frame (forward transform, selection), then the copies
int fingerprint_embed_impl(ssw_ctx* ctx, const ssw_config* cfg, const void* dev_rgb, PixFmt fmt_in, size_t w, size_t h,
                           const float* dev_marks, size_t n_copies, size_t k, void* dev_rgb_out, bool u8_out, uint32_t* dev_indices_out) {
    if (!ctx || !dev_rgb || !dev_marks || !dev_rgb_out) return SSW_ERR_BAD_ARG;
    SSW_TRY(check_config(cfg));
    if (cfg->precision != SSW_PRECISION_F64) return SSW_ERR_UNSUPPORTED;
    if (w == 0 || h == 0) return SSW_ERR_BAD_DIMS;
    if (n_copies == 0) return SSW_OK;
    const size_t plane = w * h;
    const size_t k_eff = std::min(k, plane - 1);                       // zip() truncation, :396
    CtxGuard gd(ctx);
    ssw_ctx::Lane& ws = ctx->lane[0];
    ssw_ctx::Lane::WriterPlanes pl;
    SSW_TRY(ws.writer_planes(plane * sizeof(float), pl));
    SSW_TRY(grow(ws.idx, std::max<size_t>(k_eff, 1) * sizeof(uint32_t)));
    float *y = pl.y, *pi = pl.i, *pq = pl.q, *tmp = pl.scratch;
    uint32_t* idx = dev_indices_out ? dev_indices_out : ws.idx.as<uint32_t>();
    Chain ch;
    SSW_TRY(build_forward_from_rgb(ctx, ws, cfg->precision, dev_rgb, fmt_in, 1, w, h, y, pi, pq, tmp, ch));   // Writer::new :308-313
    SSW_TRY(run_serial(ch, ctx->stream));
    if (k_eff) SSW_TRY(topk(ctx, ctx->stream, ws.sel, y, 1, w, h, cfg->ordering, k_eff, idx));              // :314 (first k only)
    return fingerprint_copies(ctx, *cfg, y, idx, k_eff, pi, pq, w, h, dev_marks, k, n_copies, dev_rgb_out, u8_out, tmp);
}

}  // namespace host
}  // namespace ssw

int ssw_fingerprint_embed(ssw_ctx* ctx, const ssw_config* cfg, const float* dev_rgb, size_t w, size_t h, const float* dev_marks,
                          size_t n_copies, size_t k, float* dev_rgb_out, uint32_t* dev_indices_out) {
    return ssw::host::fingerprint_embed_impl(ctx, cfg, dev_rgb, ssw::PixFmt::F32, w, h, dev_marks, n_copies, k, dev_rgb_out, false,
                                             dev_indices_out);
}
int ssw_fingerprint_embed_rgb8(ssw_ctx* ctx, const ssw_config* cfg, const uint8_t* dev_rgb, size_t w, size_t h, const float* dev_marks,
                               size_t n_copies, size_t k, uint8_t* dev_rgb_out, uint32_t* dev_indices_out) {
    return ssw::host::fingerprint_embed_impl(ctx, cfg, dev_rgb, ssw::PixFmt::U8, w, h, dev_marks, n_copies, k, dev_rgb_out, true,
                                             dev_indices_out);
}
