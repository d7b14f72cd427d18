// Base-reader pruning of the batch extract path.
//
// The base frame's coefficient plane is used for two things: the selection of the first k keys, and reads at those k
// indices.  A frequency column v whose every key is below the k-th key can contribute to neither, so its column
// transform is work for nothing.  The fused forward transform (EPI_FWD_COLOP) gives a bound for free: the row launches'
// energy instances add up E[v] = sum_y r(y, v)^2 of the f32 values between the passes, and by Parseval
//     c(0, v)^2 / 2 + sum_{u > 0} c(u, v)^2 = 2 H E[v]          (c = 2 sum_y r cos(pi u (2 y + 1) / 2 H), dct2d.rs:107-111)
// so every coefficient of column v has c^2 <= 4 H E[v] (u = 0 is the row that needs the 4).  boundkey(v) = G E[v] with G
// = 4 H (times the largest squared orthonormal scale for EnergyOrthogonal) rounded up by 2^-5, which covers the f32
// rounding of the sum (<= (H + 32) 2^-24 relative: H < 2^17), of the coefficient (2^-24), of the key (2^-23) and of G E.
//
// The column pass runs in two phases (BasePart::Phase1Cols / Phase2Cols): tile 0 (columns 0 .. 127) of every frame first; then this
// file's kernel takes T = a lower bound of the k-th largest key among tile 0's coefficients and marks the tiles t > 0
// that hold a column with !(boundkey < T); the second phase computes those.  A skipped coefficient has key <= boundkey <
// T <= the k-th computed key, strictly: at least k computed keys rank ahead of it, ties included, so the first k
// entries of the order do not depend on its value -- the skipped tiles are left as they are (stale workspace) and the
// selection takes the flags as a tile mask (select.hip): it reads computed tiles only.  NaN / Inf energies compare "needed"; a frame with fewer than k keys in tile 0,
// or whose T is not positive, needs every tile.  Legacy ordering (signed keys) has no bound and takes the full path.
#include <algorithm>
#include <cmath>

#include "dct_pair_common.hpp"
#include "dct_pair_colops.hpp"

namespace ssw {

namespace {

constexpr int BP_BINS = 2048;          // the top 11 bits of the sortable key, as in select.hip
constexpr int BP_THREADS = 1024;

struct BpKey {
    int ordering;
    float s[2];         // EnergyOrthogonal: scale of row 0 of the plane, of the other rows, column 0 aside (tile 0 holds it: below)
    float s0[2];        // ... of column 0
    float gain;
};

__device__ inline uint32_t bp_sortable(float v) {
    const uint32_t b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// one block per frame
__global__ __launch_bounds__(BP_THREADS) void base_prune_decide_kernel(const float* __restrict__ coef, const float* __restrict__ energy,
                                                                       unsigned W, unsigned H, BpKey kp, unsigned k,
                                                                       unsigned* __restrict__ need, unsigned long long* __restrict__ stats,
                                                                       double* __restrict__ work, double tile_flop, double tile_bytes,
                                                                       double select_bytes) {
    __shared__ unsigned hist[BP_BINS];
    __shared__ unsigned part[BP_THREADS / 64];
    __shared__ float t_sh;
    __shared__ unsigned any_sh;
    const unsigned tid = threadIdx.x, f = blockIdx.x, tiles = W / SSW_BASE_PRUNE_TILE;
    for (unsigned b = tid; b < BP_BINS; b += BP_THREADS) hist[b] = 0u;
    if (tid == 0) { t_sh = 0.0f; any_sh = 0u; }
    __syncthreads();
    // keys of tile 0, exactly as the selection forms them (index 0 is never a candidate)
    const float* plane = coef + (size_t)f * W * H;
    const unsigned quads = H * (SSW_BASE_PRUNE_TILE / 4);
    for (unsigned q = tid; q < quads; q += BP_THREADS) {
        const unsigned y = q / (SSW_BASE_PRUNE_TILE / 4), x = 4 * (q % (SSW_BASE_PRUNE_TILE / 4));
        const f32x4 c = *reinterpret_cast<const f32x4*>(plane + (size_t)y * W + x);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (y == 0 && x + e == 0) continue;
            float key;
            if (kp.ordering == SSW_ORDER_ENERGY) key = c[e] * c[e];
            else {
                const float scaled = ((x + e) == 0 ? kp.s0[y == 0] : kp.s[y == 0]) * c[e];
                key = scaled * scaled;
            }
            atomicAdd(&hist[bp_sortable(key) >> 21], 1u);
        }
    }
    __syncthreads();
    // the highest bin b with k keys or more in the bins >= b: two bins per thread, suffix sums over the threads
    const unsigned b0 = BP_BINS - 2 - 2 * tid;             // this thread's bins b0 + 1 (higher), b0
    const unsigned h1 = hist[b0 + 1], h0 = hist[b0];
    unsigned v = h1 + h0;                                  // inclusive scan over tid = over descending bins
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned u = __shfl_up(v, o);
        if ((tid & 63u) >= (unsigned)o) v += u;
    }
    if ((tid & 63u) == 63u) part[tid >> 6] = v;
    __syncthreads();
    unsigned before = 0;
    for (unsigned wv = 0; wv < (tid >> 6); ++wv) before += part[wv];
    const unsigned incl = before + v, excl = incl - h1 - h0;       // keys in bins >= b0 | > b0 + 1
    if (excl < k && incl >= k) {                                   // exactly one thread
        const unsigned bin = excl + h1 >= k ? b0 + 1 : b0;
        const uint32_t sb = (uint32_t)bin << 21;                   // lower edge of the bin in the sortable order
        // a positive edge only (bins of negative keys / zero: no bound can be below them)
        t_sh = (sb & 0x80000000u) ? __uint_as_float(sb & 0x7FFFFFFFu) : 0.0f;
    }
    __syncthreads();
    const float T = t_sh;       // 0: fewer than k keys, or nothing to compare against (edges in the denormal range count as that)
    const float* e = energy + (size_t)f * W;
    unsigned* nd = need + (size_t)f * tiles;
    for (unsigned t = tid; t < tiles; t += BP_THREADS) nd[t] = t == 0 ? 1u : 0u;
    __syncthreads();
    for (unsigned x = SSW_BASE_PRUNE_TILE + tid; x < W; x += BP_THREADS) {
        const float bound = kp.gain * e[x];
        if (!(T > 1e-30f) || !(bound < T)) { nd[x / SSW_BASE_PRUNE_TILE] = 1u; any_sh = 1u; }
    }
    __syncthreads();
    if (tid == 0 && stats) {
        unsigned computed = 0;
        for (unsigned t = 0; t < tiles; ++t) computed += nd[t];
        if (work) {                                            // (the host billed tile 0 of every frame)
            if (computed > 1) {
                atomicAdd(&work[0], (computed - 1) * tile_flop); atomicAdd(&work[1], (computed - 1) * tile_bytes);
                atomicAdd(&work[2], (computed - 1) * select_bytes);
            }
        }
        atomicAdd(&stats[0], (unsigned long long)tiles);
        atomicAdd(&stats[1], (unsigned long long)computed);
        if (any_sh) atomicAdd(&stats[2], 1ull);
    }
}

__global__ __launch_bounds__(256) void base_prune_bound_kernel(const float* __restrict__ energy, unsigned W, size_t total, float gain,
                                                               float* __restrict__ out) {
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= total) return;
    const size_t f = i / W;
    const unsigned x = (unsigned)(i - f * W), tb = x / SSW_BASE_PRUNE_TILE * SSW_BASE_PRUNE_TILE;
    out[i] = gain * energy[f * W + tb + fwd_cm128_pos(x - tb)];
}

BpKey make_key(size_t w, size_t h, int ordering) {
    float s[2][2];
    select_ortho_scales(w, h, s);
    BpKey kp;
    kp.ordering = ordering;
    kp.s[0] = s[0][0]; kp.s[1] = s[1][0];
    kp.s0[0] = s[0][1]; kp.s0[1] = s[1][1];
    kp.gain = base_prune_gain(w, h, ordering);
    return kp;
}

}  // namespace

float base_prune_gain(size_t w, size_t h, int ordering) {
    if (ordering != SSW_ORDER_ENERGY && ordering != SSW_ORDER_ENERGY_ORTHOGONAL) return 0.0f;
    if (h == 0 || h >= ((size_t)1 << 17)) return 0.0f;
    double g = 4.0 * (double)h;
    if (ordering == SSW_ORDER_ENERGY_ORTHOGONAL) {
        float s[2][2];
        select_ortho_scales(w, h, s);
        double m = 0.0;
        for (int a = 0; a < 2; ++a) for (int b = 0; b < 2; ++b) m = std::max(m, (double)s[a][b]);
        g *= m * m;
    }
    g *= 1.0 + 1.0 / 32.0;
    return nextafterf((float)g, INFINITY);
}

int launch_base_prune_decide(hipStream_t st, const float* coef, const BasePrune& bp, size_t n_frames, size_t w, size_t h) {
    if (n_frames == 0) return SSW_OK;
    if (!coef || !bp.energy || !bp.need || (reinterpret_cast<uintptr_t>(coef) & 15) != 0 || w % SSW_BASE_PRUNE_TILE != 0 || w > 0xFFFFFFull || h > 0xFFFFFFull || n_frames > 0x7FFFFFFFull ||
        bp.k == 0 || bp.k > 0xFFFFFFFFull) return SSW_ERR_BAD_ARG;
    const BpKey kp = make_key(w, h, bp.ordering);
    if (!(kp.gain > 0.0f)) return SSW_ERR_BAD_ARG;
    base_prune_decide_kernel<<<(unsigned)n_frames, BP_THREADS, 0, st>>>(coef, bp.energy, (unsigned)w, (unsigned)h, kp, (unsigned)bp.k, bp.need,
                                                                       bp.stats, bp.work, bp.tile_flop, bp.tile_bytes, bp.select_bytes);
    SSW_HIP_CHECK(hipGetLastError());
    return SSW_OK;
}

int launch_base_prune_bound(hipStream_t st, const float* energy, size_t n_frames, size_t w, size_t h, int ordering, float* out) {
    const size_t total = n_frames * w;
    if (total == 0) return SSW_OK;
    if (!energy || !out || w % SSW_BASE_PRUNE_TILE != 0) return SSW_ERR_BAD_ARG;
    const float gain = base_prune_gain(w, h, ordering);
    if (!(gain > 0.0f)) return SSW_ERR_UNSUPPORTED;
    base_prune_bound_kernel<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(energy, (unsigned)w, total, gain, out);
    SSW_HIP_CHECK(hipGetLastError());
    return SSW_OK;
}

}  // namespace ssw
