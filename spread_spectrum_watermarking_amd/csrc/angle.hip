// Finding the angle of a turned copy (ssw_find_angle_rgb8): a search over the angle of a rotation about the centre.  For every
// rung of a ladder of angles 0.25 degrees apart the original's 4 x 4 box plane is turned forward (integer bilinear taps) and its
// luma difference with the suspect's plane summed; the 4 best rungs are refined at full resolution in steps of 1/32 degree and
// the best of those is the answer.  include/ssw.h states the definition; every quantity is an integer, so nothing here depends
// on the order of a sum and the result equals the numpy restatement of tests/test_angle_cpu.py exactly.  The reference has no
// counterpart.
//
// Kernels (the planes come from locate.hip's locate_luma_kernel and locate_box_kernel):
//   angle_cost_kernel    THE HOT PATH, both factors: a block takes a tile of 32 x 32 pixels of a suspect's plane for one candidate
//                        angle (grid y: the candidate slot, grid z: the suspect).  The map is monotone in X and in Y, so the
//                        sample points of the tile's four corners bound the box of the original's plane it can touch: the box
//                        is staged in LDS and all four taps come from there.  The tile's origin is formed in 64 bits, the box's
//                        origin subtracted, and a lane adds its own offset in 32 bits -- integer adds, exact.  A lane sums
//                        |Ps - v| and its valid bit; wave, then block reduction; one 64-bit atomic add of D and one of c per block.
//   angle_keep_kernel    one block per suspect: the 4 rungs of smallest mean cost (cross-multiplied in 64 bits, ties to the
//                        smaller j) and the refinement's slot list of 60 angles, duplicates and angles outside the range marked
//                        as skipped -- on the device, so the call waits for the stream once
//   angle_final_kernel   the refined angle of smallest mean cost, ties to the smaller angle
//
// The unknown-angle row of the strength report (ssw_rotate_search_attack_rgb8): every job's frame is turned (affine.hip), the
// angle of the turned frame searched for as above, and the frame turned back by the angle FOUND.  All its suspects have one
// original, so its costs come from
//   angle_cost_shared_kernel    THE HOT PATH of that call: the turned values of a (tile, candidate) made once and compared with
//                        every member of a share-group (angle_share.hpp: at most 16 suspects turned by one matrix); per further
//                        member one aligned word load and one v_sad_u8 for four pixels.  Equal sums, so equal answers.
#include <algorithm>
#include <cmath>
#include <map>
#include <vector>

#include "angle_share.hpp"
#include "angle_tables.hpp"
#include "ssw_host.hpp"

namespace ssw {

constexpr unsigned ANG_TW = 32, ANG_TH = 32, ANG_THREADS = 256, ANG_ROWS = ANG_THREADS / ANG_TW;      // a lane: ANG_TH / ANG_ROWS pixels of a column
// The staged box.  The sample points of a tile spread over (C 31 + |S| 31) / 65536 <= 31 sqrt(2) = 43.9 plane pixels across and
// down (at 45 degrees): their floors take at most 45 values, the second tap adds one.
constexpr unsigned ANG_BOX_W = 48, ANG_BOX_H = 46;
constexpr unsigned ANG_RUNGS_MAX = 2 * ANGLE_RUNG_MAX + 1;
constexpr int32_t ANG_SKIP = INT32_MIN;
static_assert(ANG_SKIP == ANGLE_SLOT_SKIP, "angle_share.hpp reads the slot lists angle_keep_kernel writes");

struct AngleCost {
    const uint8_t* po;              // the original's plane [hr][po_pitch]
    const uint8_t* ps;              // the suspects' planes [hr][ps_pitch], ps_stride bytes apart
    size_t ps_stride;
    const int32_t* tab;             // C, S of angle a at tab[2 (a - a_lo)]
    const int32_t* slots;           // the refinement: the angle of slot y of suspect z at [z][ANGLE_SLOTS], or ANG_SKIP; null: the ladder
    unsigned long long* sums;       // [suspect][slot][2]: D, c
    uint32_t po_pitch, ps_pitch, wr, hr, w, h, f, sh, tiles_x, n_slots;
    int32_t a_lo, a_first;          // the ladder: slot y is the angle a_first + 8 y
};

__device__ inline int64_t ang_clamp(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : v > hi ? hi : v; }

// grid: (tiles of the plane, slots, suspects); block: ANG_THREADS
__global__ __launch_bounds__(ANG_THREADS) void angle_cost_kernel(AngleCost d) {
    __shared__ uint8_t s_box[ANG_BOX_H][ANG_BOX_W];
    __shared__ uint32_t s_red[2][ANG_THREADS / 64];
    const unsigned t = threadIdx.x, slot = blockIdx.y, sus = blockIdx.z;
    const int32_t a = d.slots ? d.slots[(size_t)sus * ANGLE_SLOTS + slot] : d.a_first + ANGLE_RUNG_STEP * (int32_t)slot;
    if (a == ANG_SKIP) return;                                          // (uniform)
    const int32_t C = d.tab[2 * (a - d.a_lo)], S = d.tab[2 * (a - d.a_lo) + 1];
    const uint32_t Xt = (blockIdx.x % d.tiles_x) * ANG_TW, Yt = (blockIdx.x / d.tiles_x) * ANG_TH;
    const int nx = (int)min(ANG_TW, d.wr - Xt), ny = (int)min(ANG_TH, d.hr - Yt);
    // the tile's origin, 64 bits
    const int64_t f = d.f;
    const int64_t p0 = 2 * f * Xt + f - (int64_t)d.w, q0 = 2 * f * Yt + f - (int64_t)d.h;
    const int64_t Rx0 = ((int64_t)d.w - f) * 65536 + C * p0 + S * q0;
    const int64_t Ry0 = ((int64_t)d.h - f) * 65536 - S * p0 + C * q0;
    // the four corners' offsets from it bound every pixel's: 2 f (C dx + S dy) and 2 f (-S dx + C dy)
    const int32_t f2 = 2 * (int32_t)d.f, ex = f2 * (nx - 1), ey = f2 * (ny - 1);
    const int32_t cxx = C * ex, sxy = S * ey, syx = -S * ex, cyy = C * ey;
    const int32_t oxmin = min(0, cxx) + min(0, sxy), oxmax = max(0, cxx) + max(0, sxy);
    const int32_t oymin = min(0, syx) + min(0, cyy), oymax = max(0, syx) + max(0, cyy);
    const int64_t bx0 = (Rx0 + oxmin) >> d.sh, bx1 = ((Rx0 + oxmax) >> d.sh) + 1;       // the box: plane columns bx0 .. bx1
    const int64_t by0 = (Ry0 + oymin) >> d.sh, by1 = ((Ry0 + oymax) >> d.sh) + 1;
    // no pixel of the tile is valid: X0 is one of bx0 .. bx1 - 1
    if (bx1 - 1 < 1 || bx0 > (int64_t)d.wr - 3 || by1 - 1 < 1 || by0 > (int64_t)d.hr - 3) return;      // (uniform)
    const int bw = (int)ang_clamp(bx1 - bx0 + 1, 2, ANG_BOX_W), bh = (int)ang_clamp(by1 - by0 + 1, 2, ANG_BOX_H);      // (the bound holds)
    for (int i = (int)t; i < bw * bh; i += (int)ANG_THREADS) {
        const int r = i / bw, c = i - r * bw;
        const int64_t gx = bx0 + c, gy = by0 + r;
        const bool in = gx >= 0 && gx < (int64_t)d.wr && gy >= 0 && gy < (int64_t)d.hr;
        s_box[r][c] = in ? d.po[(size_t)gy * d.po_pitch + (size_t)gx] : (uint8_t)0;
    }
    __syncthreads();
    // valid as the box sees it: 1 <= X0 <= wr - 3 with X0 = bx0 + (local X0), the local one 0 .. bw - 2
    const auto local = [](int64_t v) { return (int32_t)ang_clamp(v, -4096, 4096); };
    const int32_t lox = max(local(1 - bx0), 0), hix = min(local((int64_t)d.wr - 3 - bx0), bw - 2);
    const int32_t loy = max(local(1 - by0), 0), hiy = min(local((int64_t)d.hr - 3 - by0), bh - 2);
    const int32_t lrx0 = (int32_t)(Rx0 - bx0 * ((int64_t)1 << d.sh)), lry0 = (int32_t)(Ry0 - by0 * ((int64_t)1 << d.sh));
    const int dx = (int)(t % ANG_TW);
    const uint8_t* __restrict__ ps = d.ps + (size_t)sus * d.ps_stride + (size_t)Yt * d.ps_pitch + Xt + dx;
    uint32_t diff = 0, votes = 0;
#pragma unroll
    for (int dy = (int)(t / ANG_TW); dy < (int)ANG_TH; dy += (int)ANG_ROWS) {
        const int32_t lrx = lrx0 + f2 * (C * dx + S * dy), lry = lry0 + f2 * (C * dy - S * dx);
        const int32_t X0 = lrx >> d.sh, Y0 = lry >> d.sh;
        const bool valid = dx < nx && dy < ny && X0 >= lox && X0 <= hix && Y0 >= loy && Y0 <= hiy;
        if (valid) {
            const uint32_t fx = (uint32_t)(lrx >> (d.sh - 8)) & 255u, fy = (uint32_t)(lry >> (d.sh - 8)) & 255u;
            const uint32_t v00 = s_box[Y0][X0], v01 = s_box[Y0][X0 + 1], v10 = s_box[Y0 + 1][X0], v11 = s_box[Y0 + 1][X0 + 1];
            const uint32_t v = ((256u - fx) * (256u - fy) * v00 + fx * (256u - fy) * v01 + (256u - fx) * fy * v10 + fx * fy * v11 + 32768u) >> 16;
            const uint32_t s = ps[(size_t)dy * d.ps_pitch];
            diff += s > v ? s - v : v - s;
        }
        votes += (uint32_t)__popcll(__ballot(valid));
    }
#pragma unroll
    for (int o = 32; o; o >>= 1) diff += __shfl_down(diff, o);
    if ((t & 63) == 0) { s_red[0][t >> 6] = diff; s_red[1][t >> 6] = votes; }
    __syncthreads();
    if (t == 0) {
        uint32_t D = 0, c = 0;
#pragma unroll
        for (unsigned wv = 0; wv < ANG_THREADS / 64; ++wv) { D += s_red[0][wv]; c += s_red[1][wv]; }
        unsigned long long* out = d.sums + ((size_t)sus * d.n_slots + slot) * 2;
        if (c) { atomicAdd(out, (unsigned long long)D); atomicAdd(out + 1, (unsigned long long)c); }
    }
}

// The cost of one candidate angle for every member of a share-group (angle_share.hpp) at once -- the search inside
// ssw_rotate_search_attack_rgb8, where all suspects have one original and the copies of one rotation nearly one list of angles.
// The turned values v depend on (original, angle) only: a block stages the box and evaluates them once per (tile, candidate),
// then compares them with the plane of every member that wants the candidate.  The box bound, the 64-bit origin, the staging
// and the valid test are angle_cost_kernel's, number for number; all sums are integers, so a member's (D, c) EQUAL that kernel's.
struct AngleShared {
    const uint8_t* po;              // the original's plane [hr][po_pitch]
    const uint8_t* ps;              // the suspects' planes [hr][ps_pitch], ps_stride bytes apart; ps_pitch % 4 == 0, ps_stride % 256 == 0
    size_t ps_stride;
    const int32_t* tab;             // C, S of angle a at tab[2 (a - a_lo)]
    const ShareGroup* groups;       // grid z: the share-group sg0 + z
    const ShareCand* cands;         // the refinement: candidate y of the group at [first_cand + y]; null: the ladder, every member wants rung y
    unsigned long long* sums;       // [suspect][n_slots][2]: D, c -- at the rung (ladder), at the member's own slot (refinement)
    uint32_t po_pitch, ps_pitch, wr, hr, w, h, f, sh, tiles_x, n_slots, sg0;
    int32_t a_lo, a_first;          // the ladder: candidate y is the angle a_first + 8 y
};

// grid: (tiles of the plane, candidates, share-groups); block: ANG_THREADS.  A lane owns four consecutive pixels of one row of the
// tile, one aligned word of a member's plane (pitches are multiples of 4, tile origins of 32, plane strides of 256).
__global__ __launch_bounds__(ANG_THREADS) void angle_cost_shared_kernel(AngleShared d) {
    __shared__ uint8_t s_box[ANG_BOX_H][ANG_BOX_W];
    __shared__ uint32_t s_red[ANG_THREADS / 64][ANGLE_SHARE_MAX + 1];
    const unsigned t = threadIdx.x, cand = blockIdx.y;
    const ShareGroup& g = d.groups[d.sg0 + blockIdx.z];
    const ShareCand* sc = d.cands ? d.cands + g.first_cand + cand : nullptr;
    const int32_t a = sc ? sc->a : d.a_first + ANGLE_RUNG_STEP * (int32_t)cand;
    const uint32_t want = sc ? sc->mask : (1u << g.n_members) - 1u;     // (uniform, as everything up to the staging)
    const int32_t C = d.tab[2 * (a - d.a_lo)], S = d.tab[2 * (a - d.a_lo) + 1];
    const uint32_t Xt = (blockIdx.x % d.tiles_x) * ANG_TW, Yt = (blockIdx.x / d.tiles_x) * ANG_TH;
    const int nx = (int)min(ANG_TW, d.wr - Xt), ny = (int)min(ANG_TH, d.hr - Yt);
    // the tile's origin, 64 bits
    const int64_t f = d.f;
    const int64_t p0 = 2 * f * Xt + f - (int64_t)d.w, q0 = 2 * f * Yt + f - (int64_t)d.h;
    const int64_t Rx0 = ((int64_t)d.w - f) * 65536 + C * p0 + S * q0;
    const int64_t Ry0 = ((int64_t)d.h - f) * 65536 - S * p0 + C * q0;
    const int32_t f2 = 2 * (int32_t)d.f, ex = f2 * (nx - 1), ey = f2 * (ny - 1);
    const int32_t cxx = C * ex, sxy = S * ey, syx = -S * ex, cyy = C * ey;
    const int32_t oxmin = min(0, cxx) + min(0, sxy), oxmax = max(0, cxx) + max(0, sxy);
    const int32_t oymin = min(0, syx) + min(0, cyy), oymax = max(0, syx) + max(0, cyy);
    const int64_t bx0 = (Rx0 + oxmin) >> d.sh, bx1 = ((Rx0 + oxmax) >> d.sh) + 1;
    const int64_t by0 = (Ry0 + oymin) >> d.sh, by1 = ((Ry0 + oymax) >> d.sh) + 1;
    if (bx1 - 1 < 1 || bx0 > (int64_t)d.wr - 3 || by1 - 1 < 1 || by0 > (int64_t)d.hr - 3) return;      // (uniform) no pixel of the tile is valid
    const int bw = (int)ang_clamp(bx1 - bx0 + 1, 2, ANG_BOX_W), bh = (int)ang_clamp(by1 - by0 + 1, 2, ANG_BOX_H);
    for (int i = (int)t; i < bw * bh; i += (int)ANG_THREADS) {
        const int r = i / bw, c = i - r * bw;
        const int64_t gx = bx0 + c, gy = by0 + r;
        const bool in = gx >= 0 && gx < (int64_t)d.wr && gy >= 0 && gy < (int64_t)d.hr;
        s_box[r][c] = in ? d.po[(size_t)gy * d.po_pitch + (size_t)gx] : (uint8_t)0;
    }
    __syncthreads();
    const auto local = [](int64_t v) { return (int32_t)ang_clamp(v, -4096, 4096); };
    const int32_t lox = max(local(1 - bx0), 0), hix = min(local((int64_t)d.wr - 3 - bx0), bw - 2);
    const int32_t loy = max(local(1 - by0), 0), hiy = min(local((int64_t)d.hr - 3 - by0), bh - 2);
    const int32_t lrx0 = (int32_t)(Rx0 - bx0 * ((int64_t)1 << d.sh)), lry0 = (int32_t)(Ry0 - by0 * ((int64_t)1 << d.sh));
    // the lane's four turned values as one word, and the bytes of it that are valid
    const int dx0 = 4 * (int)(t % (ANG_TW / 4)), dy = (int)(t / (ANG_TW / 4));
    uint32_t V = 0, M = 0, votes = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int dx = dx0 + i;
        const int32_t lrx = lrx0 + f2 * (C * dx + S * dy), lry = lry0 + f2 * (C * dy - S * dx);
        const int32_t X0 = lrx >> d.sh, Y0 = lry >> d.sh;
        const bool valid = dx < nx && dy < ny && X0 >= lox && X0 <= hix && Y0 >= loy && Y0 <= hiy;
        if (valid) {
            const uint32_t fx = (uint32_t)(lrx >> (d.sh - 8)) & 255u, fy = (uint32_t)(lry >> (d.sh - 8)) & 255u;
            const uint32_t v00 = s_box[Y0][X0], v01 = s_box[Y0][X0 + 1], v10 = s_box[Y0 + 1][X0], v11 = s_box[Y0 + 1][X0 + 1];
            const uint32_t v = ((256u - fx) * (256u - fy) * v00 + fx * (256u - fy) * v01 + (256u - fx) * fy * v10 + fx * fy * v11 + 32768u) >> 16;
            V |= v << (8 * i);
            M |= 255u << (8 * i);
            ++votes;
        }
    }
    // per member: one aligned word of its plane (a valid byte lies inside the plane, so the word lies inside its row), the
    // invalid bytes replaced by v's -- they add nothing -- and four absolute differences in one instruction
    // (a lane without a valid byte reads the plane's first word and adds nothing: no divergent branch; a plane has fewer than 2^32 bytes)
    const uint32_t at = M ? (Yt + (uint32_t)dy) * d.ps_pitch + Xt + (uint32_t)dx0 : 0u;
    // Four members at a time, so that four loads are in flight and nothing but the staged values lives across a branch; a member
    // of the four that does not want the candidate reads member 0's word again and its sum is never looked at.  A lane's sum is
    // at most 4 * 255 and a wave's at most 65280: two members share a register through the wave's reduction.
#pragma unroll
    for (unsigned q = 0; q < ANGLE_SHARE_MAX / 4; ++q) {
        const uint32_t wq = (want >> (4 * q)) & 15u;
        if (wq) {                                                       // (uniform)
            uint32_t P[4];
#pragma unroll
            for (unsigned k = 0; k < 4; ++k) {
                const uint32_t member = ((wq >> k) & 1u) ? g.member[4 * q + k] : g.member[0];
                P[k] = *reinterpret_cast<const uint32_t*>(d.ps + (size_t)member * d.ps_stride + at);
            }
#pragma unroll
            for (unsigned k = 0; k < 4; ++k) P[k] = __builtin_amdgcn_sad_u8((P[k] & M) | (V & ~M), V, 0u);
            uint32_t two0 = P[0] | (P[1] << 16), two1 = P[2] | (P[3] << 16);
#pragma unroll
            for (int o = 32; o; o >>= 1) { two0 += __shfl_down(two0, o); two1 += __shfl_down(two1, o); }
            if ((t & 63) == 0) {
                s_red[t >> 6][4 * q] = two0 & 0xFFFFu; s_red[t >> 6][4 * q + 1] = two0 >> 16;
                s_red[t >> 6][4 * q + 2] = two1 & 0xFFFFu; s_red[t >> 6][4 * q + 3] = two1 >> 16;
            }
        }
    }
#pragma unroll
    for (int o = 32; o; o >>= 1) votes += __shfl_down(votes, o);
    if ((t & 63) == 0) s_red[t >> 6][ANGLE_SHARE_MAX] = votes;
    __syncthreads();
    if (t < ANGLE_SHARE_MAX && ((want >> t) & 1u)) {                    // c is counted once and added for every member
        uint32_t D = 0, c = 0;
#pragma unroll
        for (unsigned wv = 0; wv < ANG_THREADS / 64; ++wv) { D += s_red[wv][t]; c += s_red[wv][ANGLE_SHARE_MAX]; }
        const unsigned slot = sc ? sc->slot[t] : cand;
        unsigned long long* out = d.sums + ((size_t)g.member[t] * d.n_slots + slot) * 2;
        if (c) { atomicAdd(out, (unsigned long long)D); atomicAdd(out + 1, (unsigned long long)c); }
    }
}

// (D1, c1) before (D2, c2): the smaller mean, cross-multiplied (D <= 255 * 2^27, c <= 2^27)
__device__ inline bool angle_less(unsigned long long D1, unsigned long long c1, unsigned long long D2, unsigned long long c2) { return D1 * c2 < D2 * c1; }

// grid: (suspects); block: 256.  rungs [suspect][n_rungs][2]; slots [suspect][ANGLE_SLOTS]: slot 15 k + e is the angle
// 8 j_k + e - 7 of the k-th kept rung, ANG_SKIP when it lies outside 8 j0 .. 8 j1, belongs to an earlier kept rung as well, or
// there is no k-th rung.  A rung's rank is the number of rungs before it: ranks are distinct, the 4 smallest are kept.
__global__ __launch_bounds__(256) void angle_keep_kernel(const unsigned long long* __restrict__ rungs, unsigned n_rungs, int j0, int j1,
                                                         int32_t* __restrict__ slots) {
    __shared__ unsigned long long s_d[ANG_RUNGS_MAX], s_c[ANG_RUNGS_MAX];
    __shared__ int s_keep[ANGLE_KEEP];
    const unsigned t = threadIdx.x;
    const unsigned long long* r = rungs + (size_t)blockIdx.x * n_rungs * 2;
    for (unsigned i = t; i < n_rungs; i += 256) { s_d[i] = r[2 * i]; s_c[i] = r[2 * i + 1]; }
    if (t < ANGLE_KEEP) s_keep[t] = -1;
    __syncthreads();
    for (unsigned i = t; i < n_rungs; i += 256) {
        unsigned rank = 0;
        for (unsigned k = 0; k < n_rungs && rank < ANGLE_KEEP; ++k) {
            const bool before = angle_less(s_d[k], s_c[k], s_d[i], s_c[i]) || (k < i && !angle_less(s_d[i], s_c[i], s_d[k], s_c[k]));
            rank += before ? 1u : 0u;
        }
        if (rank < ANGLE_KEEP) s_keep[rank] = (int)i;
    }
    __syncthreads();
    if (t < ANGLE_SLOTS) {
        const unsigned k = t / (2 * ANGLE_NEAR + 1);
        int32_t a = ANG_SKIP;
        if (s_keep[k] >= 0) {
            a = ANGLE_RUNG_STEP * (j0 + s_keep[k]) + (int32_t)(t % (2 * ANGLE_NEAR + 1)) - ANGLE_NEAR;
            bool skip = a < ANGLE_RUNG_STEP * j0 || a > ANGLE_RUNG_STEP * j1;
            for (unsigned e = 0; e < k; ++e) {
                const int32_t other = ANGLE_RUNG_STEP * (j0 + s_keep[e]);
                skip |= s_keep[e] >= 0 && a >= other - ANGLE_NEAR && a <= other + ANGLE_NEAR;
            }
            if (skip) a = ANG_SKIP;
        }
        slots[(size_t)blockIdx.x * ANGLE_SLOTS + t] = a;
    }
}

// One thread per suspect: res[3 s] = the angle (as a 64-bit two's complement), res[3 s + 1] = its D, res[3 s + 2] = its c
__global__ __launch_bounds__(64) void angle_final_kernel(const int32_t* __restrict__ slots, const unsigned long long* __restrict__ fine, unsigned n,
                                                         unsigned long long* __restrict__ res) {
    const unsigned s = blockIdx.x * 64 + threadIdx.x;
    if (s >= n) return;
    bool have = false;
    int32_t ba = 0;
    unsigned long long bD = 0, bc = 0;
    for (unsigned t = 0; t < ANGLE_SLOTS; ++t) {
        const int32_t a = slots[(size_t)s * ANGLE_SLOTS + t];
        if (a == ANG_SKIP) continue;
        const unsigned long long D = fine[((size_t)s * ANGLE_SLOTS + t) * 2], c = fine[((size_t)s * ANGLE_SLOTS + t) * 2 + 1];
        if (!have || angle_less(D, c, bD, bc) || (a < ba && !angle_less(bD, bc, D, c))) { have = true; ba = a; bD = D; bc = c; }
    }
    res[3 * s] = (unsigned long long)(long long)ba;
    res[3 * s + 1] = bD;
    res[3 * s + 2] = bc;
}

namespace host {
namespace {

constexpr size_t ANG_GROUP_BYTES = (size_t)256 << 20;        // the planes of one group of suspects (one suspect's, if larger)
constexpr size_t ANG_GROUP_MAX = 65535;                      // grid z

size_t ang_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

int angle_launch(ssw_ctx* ctx, const AngleCost& d, size_t suspects) {
    const unsigned tiles_y = (d.hr + ANG_TH - 1) / ANG_TH;
    angle_cost_kernel<<<dim3(d.tiles_x * tiles_y, d.n_slots, (unsigned)suspects), ANG_THREADS, 0, ctx->stream>>>(d);
    SSW_HIP_CHECK(hipGetLastError());
    return SSW_OK;
}

}  // namespace
}  // namespace host
}  // namespace ssw

extern "C" int ssw_angle_table(int32_t n, int32_t* c, int32_t* s) {
    if (!c || !s) return SSW_ERR_BAD_ARG;
    ssw::angle_table(n, c, s);
    return SSW_OK;
}

extern "C" int ssw_find_angle_rgb8(ssw_ctx* ctx, const uint8_t* dev_base, const uint8_t* dev_suspects, size_t n, size_t w, size_t h,
                                   double amin, double amax, ssw_angle_found* host_found, uint64_t* host_rungs) {
    using namespace ssw;
    using namespace ssw::host;
    if (!ctx) return SSW_ERR_BAD_ARG;
    if (n == 0) return SSW_OK;
    int j0 = 0, j1 = 0;
    if (!dev_base || !dev_suspects || !host_found || !angle_rungs(amin, amax, &j0, &j1)) return SSW_ERR_BAD_ARG;
    if (w < ANGLE_SIDE_MIN || h < ANGLE_SIDE_MIN) return SSW_ERR_BAD_DIMS;
    if (w > ANGLE_PIXELS_MAX || h > ANGLE_PIXELS_MAX || w * h > ANGLE_PIXELS_MAX) return SSW_ERR_UNSUPPORTED;
    CtxGuard g(ctx);
    hipStream_t st = ctx->stream;
    const unsigned n_rungs = (unsigned)(j1 - j0 + 1);
    const int32_t a_lo = ANGLE_RUNG_STEP * j0;
    // C, S of every angle of the range: one copy
    std::vector<int32_t> tab(2 * ((size_t)ANGLE_RUNG_STEP * (n_rungs - 1) + 1));
    for (size_t i = 0; 2 * i < tab.size(); ++i) angle_table(a_lo + (int32_t)i, &tab[2 * i], &tab[2 * i + 1]);
    int32_t* dev_tab = nullptr;
    SSW_TRY(grow_as(ctx->locate.angle_tab, tab.size() * sizeof(int32_t), dev_tab));
    SSW_TRY(upload(ctx, dev_tab, tab.data(), tab.size() * sizeof(int32_t), st));
    untimed_work(ctx);
    // answers [n][3] | rung sums [n][n_rungs][2] | refinement sums [n][ANGLE_SLOTS][2] | slot lists [n][ANGLE_SLOTS] i32
    const size_t head = n * (3 + 2 * (size_t)n_rungs), words = head + n * 2 * ANGLE_SLOTS;
    unsigned long long* res = nullptr;
    SSW_TRY(grow_as(ctx->locate.angle_sums, words * sizeof(unsigned long long) + n * ANGLE_SLOTS * sizeof(int32_t), res));
    unsigned long long *rungs = res + 3 * n, *fine = res + head;
    int32_t* slots = reinterpret_cast<int32_t*>(res + words);
    // planes: luma rows of lp bytes, box rows of qp bytes
    const size_t wq = w / 4, hq = h / 4;
    const unsigned lp = (unsigned)ang_up(w, 4), qp = (unsigned)ang_up(wq, 4);
    const size_t sl = ang_up((size_t)lp * h, 256), sq = ang_up((size_t)qp * hq, 256);
    const size_t per = std::min(n, std::min(ANG_GROUP_MAX, std::max<size_t>(1, ANG_GROUP_BYTES / (sl + sq))));
    uint8_t *lo = nullptr, *lo4 = nullptr, *ws = nullptr;
    SSW_TRY(grow_as(ctx->locate.luma, (size_t)lp * h + 16, lo));
    SSW_TRY(grow_as(ctx->locate.phases, (size_t)qp * hq + 16, lo4));
    SSW_TRY(grow_as(ctx->locate.group, per * (sl + sq) + 16, ws));
    {
        // plane bytes: made once, read once per candidate
        const double px = (double)w * h, pq = (double)wq * hq;
        StageTimer t(ctx, SSW_STAGE_LOCATE, st, (double)(n + 1) * (4.0 * px + 2.0 * pq) + (double)n * 2.0 * (n_rungs * pq + ANGLE_SLOTS * px));
        SSW_HIP_CHECK(hipMemsetAsync(res, 0, words * sizeof(unsigned long long), st));
        SSW_TRY(locate_luma_planes(ctx, dev_base, 1, w, h, lo, 0, lp));
        SSW_TRY(locate_box4_planes(ctx, lo, 0, lp, 1, w, h, lo4, 0, qp));
        for (size_t g0 = 0; g0 < n; g0 += per) {
            const size_t m = std::min(per, n - g0);
            uint8_t *sus_l = ws, *sus_q = ws + per * sl;
            SSW_TRY(locate_luma_planes(ctx, dev_suspects + g0 * w * h * 3, m, w, h, sus_l, sl, lp));
            SSW_TRY(locate_box4_planes(ctx, sus_l, sl, lp, m, w, h, sus_q, sq, qp));
            AngleCost d{};
            d.tab = dev_tab; d.a_lo = a_lo; d.a_first = a_lo; d.w = (uint32_t)w; d.h = (uint32_t)h;
            // the ladder: every rung at f = 4
            d.po = lo4; d.po_pitch = qp; d.ps = sus_q; d.ps_stride = sq; d.ps_pitch = qp; d.wr = (uint32_t)wq; d.hr = (uint32_t)hq;
            d.f = 4; d.sh = 19; d.tiles_x = (uint32_t)((wq + ANG_TW - 1) / ANG_TW); d.n_slots = n_rungs;
            d.slots = nullptr; d.sums = rungs + g0 * 2 * n_rungs;
            {
                StageTimer tc(ctx, SSW_STAGE_LOCATE_COARSE, st);          // the coarse pass, as ssw_locate_rgb8 bills its own
                if (ctx->timing) ctx->stage_work[SSW_STAGE_LOCATE_COARSE] += (double)m * n_rungs * pq;       // byte differences, not bytes
                SSW_TRY(angle_launch(ctx, d, m));
            }
            angle_keep_kernel<<<(unsigned)m, 256, 0, st>>>(rungs + g0 * 2 * n_rungs, n_rungs, j0, j1, slots + g0 * ANGLE_SLOTS);
            SSW_HIP_CHECK(hipGetLastError());
            untimed_work(ctx);                                          // (the call's own timer ends behind everything, not with the ladder's)
            // the refinement: the slot lists at f = 1
            d.po = lo; d.po_pitch = lp; d.ps = sus_l; d.ps_stride = sl; d.ps_pitch = lp; d.wr = (uint32_t)w; d.hr = (uint32_t)h;
            d.f = 1; d.sh = 17; d.tiles_x = (uint32_t)((w + ANG_TW - 1) / ANG_TW); d.n_slots = ANGLE_SLOTS;
            d.slots = slots + g0 * ANGLE_SLOTS; d.sums = fine + g0 * 2 * ANGLE_SLOTS;
            SSW_TRY(angle_launch(ctx, d, m));
            angle_final_kernel<<<(unsigned)((m + 63) / 64), 64, 0, st>>>(slots + g0 * ANGLE_SLOTS, fine + g0 * 2 * ANGLE_SLOTS, (unsigned)m, res + 3 * g0);
            SSW_HIP_CHECK(hipGetLastError());
        }
    }
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the sums come down as they are");
    std::vector<uint64_t> got(head);
    SSW_HIP_CHECK(hipMemcpyAsync(got.data(), res, head * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    untimed_work(ctx);
    SSW_HIP_CHECK(hipStreamSynchronize(st));
    for (size_t i = 0; i < n; ++i)
        host_found[i] = ssw_angle_found{(int32_t)(int64_t)got[3 * i], n_rungs, got[3 * i + 1], got[3 * i + 2]};
    if (host_rungs) std::copy(got.begin() + 3 * n, got.end(), host_rungs);
    return SSW_OK;
}

// ---- the unknown-angle row of the strength report ----------------------------------------------------------------------------
namespace ssw {
namespace host {
namespace {

bool rs_finite(const double* m, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(m[i])) return false;
    return true;
}
bool rs_overlaps(const uint8_t* a, size_t na, const uint8_t* b, size_t nb) {
    const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
    return pa < pb + nb && pb < pa + na;
}

int angle_shared_launch(ssw_ctx* ctx, const AngleShared& d, unsigned cands, unsigned share_groups) {
    const unsigned tiles_y = (d.hr + ANG_TH - 1) / ANG_TH;
    angle_cost_shared_kernel<<<dim3(d.tiles_x * tiles_y, cands, share_groups), ANG_THREADS, 0, ctx->stream>>>(d);
    SSW_HIP_CHECK(hipGetLastError());
    return SSW_OK;
}

}  // namespace
}  // namespace host
}  // namespace ssw

extern "C" int ssw_rotate_search_attack_rgb8(ssw_ctx* ctx, const uint8_t* dev_base, const uint8_t* dev_frames, size_t n_frames, size_t w, size_t h,
                                             const ssw_rotate_job* jobs, size_t n_jobs, double amin, double amax, uint8_t* dev_out,
                                             uint8_t* dev_turned, ssw_angle_found* host_found, uint64_t* host_rungs, uint64_t* host_kept) {
    using namespace ssw;
    using namespace ssw::host;
    if (!ctx) return SSW_ERR_BAD_ARG;
    if (n_jobs == 0) return SSW_OK;
    int j0 = 0, j1 = 0;
    if (!dev_base || !dev_frames || !jobs || !dev_out || !host_found || !host_kept || !angle_rungs(amin, amax, &j0, &j1)) return SSW_ERR_BAD_ARG;
    if (w < ANGLE_SIDE_MIN || h < ANGLE_SIDE_MIN || w > 65535 || h > 65535) return SSW_ERR_BAD_DIMS;
    if (w * h > ANGLE_PIXELS_MAX) return SSW_ERR_UNSUPPORTED;
    for (size_t i = 0; i < n_jobs; ++i)
        if (jobs[i].frame >= n_frames || jobs[i].filter > (uint32_t)SSW_AFFINE_BICUBIC || !rs_finite(jobs[i].forward, 6)) return SSW_ERR_BAD_ARG;
    const size_t fb = w * h * 3, N = n_jobs;
    if (rs_overlaps(dev_frames, n_frames * fb, dev_out, N * fb) || rs_overlaps(dev_base, fb, dev_out, N * fb)) return SSW_ERR_BAD_ARG;
    if (dev_turned && (rs_overlaps(dev_frames, n_frames * fb, dev_turned, N * fb) || rs_overlaps(dev_base, fb, dev_turned, N * fb) ||
                       rs_overlaps(dev_out, N * fb, dev_turned, N * fb))) return SSW_ERR_BAD_ARG;
    CtxGuard g(ctx);
    hipStream_t st = ctx->stream;
    const unsigned n_rungs = (unsigned)(j1 - j0 + 1);
    const int32_t a_lo = ANGLE_RUNG_STEP * j0;
    std::vector<int32_t> tab(2 * ((size_t)ANGLE_RUNG_STEP * (n_rungs - 1) + 1));
    for (size_t i = 0; 2 * i < tab.size(); ++i) angle_table(a_lo + (int32_t)i, &tab[2 * i], &tab[2 * i + 1]);
    int32_t* dev_tab = nullptr;
    SSW_TRY(grow_as(ctx->locate.angle_tab, tab.size() * sizeof(int32_t), dev_tab));
    SSW_TRY(upload(ctx, dev_tab, tab.data(), tab.size() * sizeof(int32_t), st));
    untimed_work(ctx);
    // answers [N][3] | rung sums [N][n_rungs][2] | refinement sums [N][ANGLE_SLOTS][2] | kept counts [N] | slot lists [N][ANGLE_SLOTS] i32
    // | share-groups [N] | their candidates [N ANGLE_SLOTS]
    const size_t head = N * (3 + 2 * (size_t)n_rungs), words = head + N * 2 * ANGLE_SLOTS + N;
    unsigned long long* res = nullptr;
    SSW_TRY(grow_as(ctx->locate.angle_sums, words * sizeof(unsigned long long) + N * ANGLE_SLOTS * sizeof(int32_t) + N * sizeof(ShareGroup) +
                                                N * ANGLE_SLOTS * sizeof(ShareCand), res));
    unsigned long long *rungs = res + 3 * N, *fine = res + head, *kept = fine + N * 2 * ANGLE_SLOTS;
    int32_t* slots = reinterpret_cast<int32_t*>(res + words);
    ShareGroup* dev_groups = reinterpret_cast<ShareGroup*>(slots + N * ANGLE_SLOTS);
    ShareCand* dev_cands = reinterpret_cast<ShareCand*>(dev_groups + N);
    // planes: luma rows of lp bytes, box rows of qp bytes; a group: the turned frames and their planes, ANG_GROUP_BYTES at most
    const size_t wq = w / 4, hq = h / 4;
    const unsigned lp = (unsigned)ang_up(w, 4), qp = (unsigned)ang_up(wq, 4);
    const size_t sl = ang_up((size_t)lp * h, 256), sq = ang_up((size_t)qp * hq, 256);
    const size_t per = std::min(N, std::min(ANG_GROUP_MAX, std::max<size_t>(1, ANG_GROUP_BYTES / (fb + sl + sq))));
    uint8_t *lo = nullptr, *lo4 = nullptr, *ws = nullptr, *turned_ws = nullptr;
    SSW_TRY(grow_as(ctx->locate.luma, (size_t)lp * h + 16, lo));
    SSW_TRY(grow_as(ctx->locate.phases, (size_t)qp * hq + 16, lo4));
    SSW_TRY(grow_as(ctx->locate.group, per * (sl + sq) + 16, ws));
    if (!dev_turned) SSW_TRY(grow_as(ctx->shared.affine, per * fb, turned_ws));
    const double px = (double)w * h, pq = (double)wq * hq;
    {
        StageTimer t(ctx, SSW_STAGE_LOCATE, st, 4.0 * px + 2.0 * pq);
        SSW_HIP_CHECK(hipMemsetAsync(res, 0, words * sizeof(unsigned long long), st));
        SSW_TRY(locate_luma_planes(ctx, dev_base, 1, w, h, lo, 0, lp));
        SSW_TRY(locate_box4_planes(ctx, lo, 0, lp, 1, w, h, lo4, 0, qp));
    }
    std::map<int32_t, size_t> kept_at;                       // the angle found -> where its mask is counted
    std::vector<int32_t> found_n(N);
    std::vector<int32_t> host_slots;
    std::vector<uint64_t> got;
    std::vector<ShareCand> cands;
    for (size_t g0 = 0; g0 < N; g0 += per) {
        const size_t m = std::min(per, N - g0);
        uint8_t* T = dev_turned ? dev_turned + g0 * fb : turned_ws;
        uint8_t *sus_l = ws, *sus_q = ws + per * sl;
        {
            // the turn: consecutive jobs of one filter, fill and matrix in one set of launches
            StageTimer t(ctx, SSW_STAGE_RESIZE, st, (double)m * 2.0 * (double)fb);
            for (size_t i0 = g0; i0 < g0 + m;) {
                const ssw_rotate_job& j = jobs[i0];
                size_t i1 = i0 + 1;
                while (i1 < g0 + m && jobs[i1].filter == j.filter && std::equal(j.fill, j.fill + 3, jobs[i1].fill) &&
                       std::equal(j.forward, j.forward + 6, jobs[i1].forward)) ++i1;
                std::vector<uint32_t> frames(i1 - i0);
                for (size_t i = i0; i < i1; ++i) frames[i - i0] = jobs[i].frame;
                SSW_TRY(affine_frames(ctx, dev_frames, fb, frames.data(), i1 - i0, w, h, j.forward, nullptr, (int)j.filter, j.fill, nullptr, T + (i0 - g0) * fb));
                i0 = i1;
            }
        }
        std::vector<const double*> keys(m);
        for (size_t i = 0; i < m; ++i) keys[i] = jobs[g0 + i].forward;
        std::vector<ShareGroup> groups = angle_share_groups(keys);
        SSW_TRY(upload(ctx, dev_groups, groups.data(), groups.size() * sizeof(ShareGroup), st));
        untimed_work(ctx);
        AngleShared d{};
        d.tab = dev_tab; d.a_lo = a_lo; d.a_first = a_lo; d.w = (uint32_t)w; d.h = (uint32_t)h; d.groups = dev_groups;
        {
            StageTimer t(ctx, SSW_STAGE_LOCATE, st, (double)m * (4.0 * px + 2.0 * pq + 2.0 * n_rungs * pq));
            SSW_TRY(locate_luma_planes(ctx, T, m, w, h, sus_l, sl, lp));
            SSW_TRY(locate_box4_planes(ctx, sus_l, sl, lp, m, w, h, sus_q, sq, qp));
            // the ladder: every rung at f = 4, every member of a share-group
            d.po = lo4; d.po_pitch = qp; d.ps = sus_q; d.ps_stride = sq; d.ps_pitch = qp; d.wr = (uint32_t)wq; d.hr = (uint32_t)hq;
            d.f = 4; d.sh = 19; d.tiles_x = (uint32_t)((wq + ANG_TW - 1) / ANG_TW); d.n_slots = n_rungs;
            d.cands = nullptr; d.sums = rungs + g0 * 2 * n_rungs; d.sg0 = 0;
            {
                StageTimer tc(ctx, SSW_STAGE_LOCATE_COARSE, st);
                if (ctx->timing) ctx->stage_work[SSW_STAGE_LOCATE_COARSE] += (double)m * n_rungs * pq;
                SSW_TRY(angle_shared_launch(ctx, d, n_rungs, (unsigned)groups.size()));
            }
            angle_keep_kernel<<<(unsigned)m, 256, 0, st>>>(rungs + g0 * 2 * n_rungs, n_rungs, j0, j1, slots + g0 * ANGLE_SLOTS);
            SSW_HIP_CHECK(hipGetLastError());
        }
        // the first wait of the group: the slot lists come down, the host forms the unions and who wants what
        host_slots.resize(m * ANGLE_SLOTS);
        SSW_TRY(download(ctx, host_slots.data(), slots + g0 * ANGLE_SLOTS, m * ANGLE_SLOTS * sizeof(int32_t), st));
        angle_share_cands(host_slots.data(), groups, cands);
        SSW_TRY(upload(ctx, dev_groups, groups.data(), groups.size() * sizeof(ShareGroup), st));
        SSW_TRY(upload(ctx, dev_cands, cands.data(), cands.size() * sizeof(ShareCand), st));
        untimed_work(ctx);
        {
            // the refinement at f = 1: one launch per share-group, its grid exactly the group's candidates
            StageTimer t(ctx, SSW_STAGE_LOCATE, st, (double)cands.size() * px + (double)m * ANGLE_SLOTS * px);
            d.po = lo; d.po_pitch = lp; d.ps = sus_l; d.ps_stride = sl; d.ps_pitch = lp; d.wr = (uint32_t)w; d.hr = (uint32_t)h;
            d.f = 1; d.sh = 17; d.tiles_x = (uint32_t)((w + ANG_TW - 1) / ANG_TW); d.n_slots = ANGLE_SLOTS;
            d.cands = dev_cands; d.sums = fine + g0 * 2 * ANGLE_SLOTS;
            for (size_t s = 0; s < groups.size(); ++s) {
                if (!groups[s].n_cands) continue;
                d.sg0 = (uint32_t)s;
                SSW_TRY(angle_shared_launch(ctx, d, groups[s].n_cands, 1));
            }
            angle_final_kernel<<<(unsigned)((m + 63) / 64), 64, 0, st>>>(slots + g0 * ANGLE_SLOTS, fine + g0 * 2 * ANGLE_SLOTS, (unsigned)m, res + 3 * g0);
            SSW_HIP_CHECK(hipGetLastError());
        }
        // the second wait: the answers, which shape the undoing
        static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the sums come down as they are");
        got.resize(3 * m);
        SSW_TRY(download(ctx, got.data(), res + 3 * g0, 3 * m * sizeof(uint64_t), st));
        untimed_work(ctx);
        for (size_t i = 0; i < m; ++i) {
            host_found[g0 + i] = ssw_angle_found{(int32_t)(int64_t)got[3 * i], n_rungs, got[3 * i + 1], got[3 * i + 2]};
            found_n[g0 + i] = host_found[g0 + i].n;
        }
        {
            // the undoing by the angle found, as ssw_unrotate_rgb8 does it for Rotate(n / 32)'s job: consecutive jobs of one answer together
            StageTimer t(ctx, SSW_STAGE_RESIZE, st, (double)m * 2.0 * (double)fb);
            for (size_t i0 = g0; i0 < g0 + m;) {
                size_t i1 = i0 + 1;
                while (i1 < g0 + m && found_n[i1] == found_n[i0]) ++i1;
                double F[6], B[6];
                rotation_matrix((double)found_n[i0] / ANGLE_PER_DEGREE, w, h, F);
                rotation_matrix(-(double)found_n[i0] / ANGLE_PER_DEGREE, w, h, B);
                if (affine_is_identity(F) && affine_is_identity(B)) {
                    SSW_HIP_CHECK(hipMemcpyAsync(dev_out + i0 * fb, T + (i0 - g0) * fb, (i1 - i0) * fb, hipMemcpyDeviceToDevice, st));
                } else {
                    std::vector<uint32_t> own(i1 - i0);
                    for (size_t i = i0; i < i1; ++i) own[i - i0] = (uint32_t)(i - g0);
                    SSW_TRY(affine_frames(ctx, T, fb, own.data(), i1 - i0, w, h, B, F, AFFINE_BICUBIC, nullptr, dev_base, dev_out + i0 * fb));
                    if (!kept_at.count(found_n[i0])) {
                        const size_t at = kept_at.size();
                        kept_at[found_n[i0]] = at;
                        SSW_TRY(affine_kept_enqueue(ctx, w, h, B, F, kept + at));
                    }
                }
                i0 = i1;
            }
        }
    }
    // the call's last wait: the rung sums and the masks' counts
    std::vector<uint64_t> counts(kept_at.size());
    if (!counts.empty()) SSW_HIP_CHECK(hipMemcpyAsync(counts.data(), kept, counts.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    if (host_rungs) SSW_HIP_CHECK(hipMemcpyAsync(host_rungs, rungs, N * 2 * (size_t)n_rungs * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    untimed_work(ctx);
    SSW_HIP_CHECK(hipStreamSynchronize(st));
    for (size_t i = 0; i < N; ++i) {
        const auto it = kept_at.find(found_n[i]);
        host_kept[i] = it == kept_at.end() ? (uint64_t)w * h : counts[it->second];
    }
    return SSW_OK;
}
