// Finding the angle of a turned copy (ssw_find_angle_rgb8): a search over the angle of a rotation about the centre.  For every
// rung of a ladder of angles 0.25 degrees apart the original's 4 x 4 box plane is turned forward (integer bilinear taps) and its
// luma difference with the suspect's plane summed; the 4 best rungs are refined at full resolution in steps of 1/32 degree and
// the best of those is the answer.  include/ssw.h states the definition; every quantity is an integer, so nothing here depends
// on the order of a sum and the result equals the numpy restatement of tests/test_angle_cpu.py exactly.  The reference has no
// counterpart.
//
// Kernels (the planes come from locate.hip's locate_luma_kernel and locate_box_kernel):
//   angle_cost_kernel    THE HOT PATH, both factors: a block takes a tile of a suspect's plane for one candidate angle (grid y:
//                        the candidate slot, grid z: the suspect) and the staged box of the original's plane: turned_tile.hpp.
//                        A lane sums |Ps - v| and its valid bit, a pixel per row step; wave, then block reduction; one 64-bit
//                        atomic add of D and one of c per block.
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
#include "turned_tile.hpp"

namespace ssw {

constexpr unsigned ANG_ROWS = TURN_THREADS / TURN_TILE_W;         // angle_cost_kernel's lane: TURN_TILE_H / ANG_ROWS pixels of a column
constexpr unsigned ANG_RUNGS_MAX = 2 * ANGLE_RUNG_MAX + 1;
constexpr int32_t ANG_SKIP = INT32_MIN;
static_assert(ANG_SKIP == ANGLE_SLOT_SKIP, "angle_share.hpp reads the slot lists angle_keep_kernel writes");

// A level of the search, the part of a descriptor both cost kernels read: the ladder's (f = 4, sh = 19, the 4 x 4 box planes) or
// the refinement's (f = 1, sh = 17, the luma planes)
struct AngleLevel {
    const uint8_t* po;              // the original's plane [hr][po_pitch]
    const uint8_t* ps;              // the suspects' planes [hr][ps_pitch], ps_stride bytes apart
    size_t ps_stride;
    const int32_t* tab;             // C, S of angle a at tab[2 (a - a_lo)]
    unsigned long long* sums;       // [suspect][n_slots][2]: D, c
    uint32_t po_pitch, ps_pitch, wr, hr, w, h, f, sh, tiles_x, n_slots;
    int32_t a_lo, a_first;          // the ladder: slot y is the angle a_first + 8 y
};
struct AngleCost {
    AngleLevel lv;
    const int32_t* slots;           // the refinement: the angle of slot y of suspect z at [z][ANGLE_SLOTS], or ANG_SKIP; null: the ladder
};
struct AngleShared {                // ps_pitch % 4 == 0, ps_stride % 256 == 0
    AngleLevel lv;                  // sums: at the rung (ladder), at the member's own slot (refinement)
    const ShareGroup* groups;       // grid z: the share-group sg0 + z
    const ShareCand* cands;         // the refinement: candidate y of the group at [first_cand + y]; null: the ladder, every member wants rung y
    uint32_t sg0;
};

// A block of either cost kernel: the tile blockIdx.x of the candidate angle, and the valid window 1 <= X0 <= wr - 3 as the box
// sees it -- X0 = bx0 + (local X0), the local one 0 .. bw - 2
struct AngleBlock {
    Turn m;
    TurnedTile tl;
    uint32_t Xt, Yt;
    int nx, ny;
    int32_t lox, hix, loy, hiy;
};

// stages the box; false, and nothing staged: no pixel of the tile is valid (uniform)
__device__ __forceinline__ bool angle_block(const AngleLevel& d, int32_t a, TurnedBox& s_box, AngleBlock& b) {
    b.m = Turn{d.tab[2 * (a - d.a_lo)], d.tab[2 * (a - d.a_lo) + 1], d.f, d.sh, d.w, d.h, d.w, d.h};
    b.Xt = (blockIdx.x % d.tiles_x) * TURN_TILE_W; b.Yt = (blockIdx.x / d.tiles_x) * TURN_TILE_H;
    b.nx = (int)min(TURN_TILE_W, d.wr - b.Xt); b.ny = (int)min(TURN_TILE_H, d.hr - b.Yt);
    b.tl = turned_tile(b.m, b.Xt, b.Yt, b.nx, b.ny);
    const TurnedTile& tl = b.tl;
    if (tl.bx1 - 1 < 1 || tl.bx0 > (int64_t)d.wr - 3 || tl.by1 - 1 < 1 || tl.by0 > (int64_t)d.hr - 3) return false;      // X0 is one of bx0 .. bx1 - 1
    turned_stage(s_box, d.po, d.po_pitch, d.wr, d.hr, tl);
    const auto local = [](int64_t v) { return (int32_t)turn_clamp(v, -4096, 4096); };
    b.lox = max(local(1 - tl.bx0), 0); b.hix = min(local((int64_t)d.wr - 3 - tl.bx0), tl.bw - 2);
    b.loy = max(local(1 - tl.by0), 0); b.hiy = min(local((int64_t)d.hr - 3 - tl.by0), tl.bh - 2);
    return true;
}

// pixel (dx, dy) of the tile: whether it is valid, and then its turned value
__device__ __forceinline__ bool angle_value(const AngleBlock& b, const TurnedBox& s_box, int dx, int dy, uint32_t& v) {
    int32_t lrx, lry;
    turned_pixel(b.m, b.tl, dx, dy, &lrx, &lry);
    const int32_t X0 = lrx >> b.m.shift, Y0 = lry >> b.m.shift;
    const bool valid = dx < b.nx && dy < b.ny && X0 >= b.lox && X0 <= b.hix && Y0 >= b.loy && Y0 <= b.hiy;
    if (valid) v = turned_value(s_box, b.m, X0, Y0, lrx, lry);
    return valid;
}

// grid: (tiles of the plane, slots, suspects); block: TURN_THREADS
__global__ __launch_bounds__(TURN_THREADS) void angle_cost_kernel(AngleCost d) {
    __shared__ TurnedBox s_box;
    __shared__ uint32_t s_red[2][TURN_THREADS / 64];
    const AngleLevel& lv = d.lv;
    const unsigned t = threadIdx.x, slot = blockIdx.y, sus = blockIdx.z;
    const int32_t a = d.slots ? d.slots[(size_t)sus * ANGLE_SLOTS + slot] : lv.a_first + ANGLE_RUNG_STEP * (int32_t)slot;
    if (a == ANG_SKIP) return;                                          // (uniform)
    AngleBlock b;
    if (!angle_block(lv, a, s_box, b)) return;
    const int dx = (int)(t % TURN_TILE_W);
    const uint8_t* __restrict__ ps = lv.ps + (size_t)sus * lv.ps_stride + (size_t)b.Yt * lv.ps_pitch + b.Xt + dx;
    uint32_t diff = 0, votes = 0;
#pragma unroll
    for (int dy = (int)(t / TURN_TILE_W); dy < (int)TURN_TILE_H; dy += (int)ANG_ROWS) {
        uint32_t v = 0;
        const bool valid = angle_value(b, s_box, dx, dy, v);
        if (valid) {
            const uint32_t s = ps[(size_t)dy * lv.ps_pitch];
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
        for (unsigned wv = 0; wv < TURN_THREADS / 64; ++wv) { D += s_red[0][wv]; c += s_red[1][wv]; }
        unsigned long long* out = lv.sums + ((size_t)sus * lv.n_slots + slot) * 2;
        if (c) { atomicAdd(out, (unsigned long long)D); atomicAdd(out + 1, (unsigned long long)c); }
    }
}

// The cost of one candidate angle for every member of a share-group (angle_share.hpp) at once -- the search inside
// ssw_rotate_search_attack_rgb8, where all suspects have one original and the copies of one rotation nearly one list of angles.
// The turned values v depend on (original, angle) only: a block stages the box and evaluates them once per (tile, candidate)
// -- angle_block and angle_value, as angle_cost_kernel --, then compares them with the plane of every member that wants the
// candidate.  All sums are integers, so a member's (D, c) EQUAL that kernel's.
// grid: (tiles of the plane, candidates, share-groups); block: TURN_THREADS.  A lane owns four consecutive pixels of one row of the
// tile, one aligned word of a member's plane (pitches are multiples of 4, tile origins of 32, plane strides of 256).
__global__ __launch_bounds__(TURN_THREADS) void angle_cost_shared_kernel(AngleShared d) {
    __shared__ TurnedBox s_box;
    __shared__ uint32_t s_red[TURN_THREADS / 64][ANGLE_SHARE_MAX + 1];
    const AngleLevel& lv = d.lv;
    const unsigned t = threadIdx.x, cand = blockIdx.y;
    const ShareGroup& g = d.groups[d.sg0 + blockIdx.z];
    const ShareCand* sc = d.cands ? d.cands + g.first_cand + cand : nullptr;
    const int32_t a = sc ? sc->a : lv.a_first + ANGLE_RUNG_STEP * (int32_t)cand;
    const uint32_t want = sc ? sc->mask : (1u << g.n_members) - 1u;     // (uniform, as everything up to the staging)
    AngleBlock b;
    if (!angle_block(lv, a, s_box, b)) return;
    // the lane's four turned values as one word, and the bytes of it that are valid
    const int dx0 = 4 * (int)(t % (TURN_TILE_W / 4)), dy = (int)(t / (TURN_TILE_W / 4));
    uint32_t V = 0, M = 0, votes = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        uint32_t v = 0;
        if (angle_value(b, s_box, dx0 + i, dy, v)) {
            V |= v << (8 * i);
            M |= 255u << (8 * i);
            ++votes;
        }
    }
    // per member: one aligned word of its plane (a valid byte lies inside the plane, so the word lies inside its row), the
    // invalid bytes replaced by v's -- they add nothing -- and four absolute differences in one instruction
    // (a lane without a valid byte reads the plane's first word and adds nothing: no divergent branch; a plane has fewer than 2^32 bytes)
    const uint32_t at = M ? (b.Yt + (uint32_t)dy) * lv.ps_pitch + b.Xt + (uint32_t)dx0 : 0u;
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
                P[k] = *reinterpret_cast<const uint32_t*>(lv.ps + (size_t)member * lv.ps_stride + at);
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
        for (unsigned wv = 0; wv < TURN_THREADS / 64; ++wv) { D += s_red[wv][t]; c += s_red[wv][ANGLE_SHARE_MAX]; }
        const unsigned slot = sc ? sc->slot[t] : cand;
        unsigned long long* out = lv.sums + ((size_t)g.member[t] * lv.n_slots + slot) * 2;
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

constexpr size_t ANG_GROUP_BYTES = (size_t)256 << 20;        // the workspace of one group of suspects (one suspect's, if larger)
constexpr size_t ANG_GROUP_MAX = 65535;                      // grid z

bool rs_finite(const double* m, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(m[i])) return false;
    return true;
}
bool rs_overlaps(const uint8_t* a, size_t na, const uint8_t* b, size_t nb) {
    const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
    return pa < pb + nb && pb < pa + na;
}

dim3 angle_grid(const AngleLevel& lv, unsigned y, unsigned z) { return dim3(lv.tiles_x * ((lv.hr + TURN_TILE_H - 1) / TURN_TILE_H), y, z); }

int angle_launch(ssw_ctx* ctx, const AngleCost& d, size_t suspects) {
    angle_cost_kernel<<<angle_grid(d.lv, d.lv.n_slots, (unsigned)suspects), TURN_THREADS, 0, ctx->stream>>>(d);
    SSW_HIP_CHECK(hipGetLastError());
    return SSW_OK;
}

int angle_shared_launch(ssw_ctx* ctx, const AngleShared& d, unsigned cands, unsigned share_groups) {
    angle_cost_shared_kernel<<<angle_grid(d.lv, cands, share_groups), TURN_THREADS, 0, ctx->stream>>>(d);
    SSW_HIP_CHECK(hipGetLastError());
    return SSW_OK;
}

// What the two searches set up alike, once per call: the table, the layout of locate.angle_sums, the planes' geometry and the
// workspace of a group of `per` suspects.  Nothing here is timed; the callers own every StageTimer.
struct AngleSearch {
    ssw_ctx* ctx;
    size_t n, w, h, wq, hq;
    int j0, j1;
    unsigned n_rungs;
    int32_t a_lo;
    int32_t* dev_tab = nullptr;          // C, S of every angle of the range
    // locate.angle_sums: answers [n][3] | rung sums [n][n_rungs][2] | refinement sums [n][ANGLE_SLOTS][2] | kept counts [n] -- all
    // 64-bit, `zeroed` bytes of them -- | slot lists [n][ANGLE_SLOTS] i32 | share-groups [n] | their candidates [n ANGLE_SLOTS];
    // the counts, groups and candidates for the strength report only
    unsigned long long *res = nullptr, *rungs = nullptr, *fine = nullptr, *kept = nullptr;
    int32_t* slots = nullptr;
    ShareGroup* groups = nullptr;
    ShareCand* cands = nullptr;
    size_t zeroed = 0;
    // planes: luma rows of lp bytes, box rows of qp bytes, a suspect's planes sl and sq bytes apart
    unsigned lp, qp;
    size_t sl, sq, per;
    double px, pq;                       // a plane's pixels
    uint8_t *lo = nullptr, *lo4 = nullptr, *sus_l = nullptr, *sus_q = nullptr;

    AngleSearch(ssw_ctx* c, size_t n_, size_t w_, size_t h_, int j0_, int j1_)
        : ctx(c), n(n_), w(w_), h(h_), wq(w_ / 4), hq(h_ / 4), j0(j0_), j1(j1_), n_rungs((unsigned)(j1_ - j0_ + 1)), a_lo(ANGLE_RUNG_STEP * j0_),
          lp((unsigned)round_up(w_, 4)), qp((unsigned)round_up(w_ / 4, 4)), sl(round_up((size_t)lp * h_, 256)), sq(round_up((size_t)qp * (h_ / 4), 256)),
          px((double)w_ * h_), pq((double)(w_ / 4) * (h_ / 4)) {}

    // `extra`: what a suspect takes of a group's bytes beside its two planes; `report`: the strength report's call
    int init(size_t extra, bool report) {
        hipStream_t st = ctx->stream;
        std::vector<int32_t> tab(2 * ((size_t)ANGLE_RUNG_STEP * (n_rungs - 1) + 1));
        for (size_t i = 0; 2 * i < tab.size(); ++i) angle_table(a_lo + (int32_t)i, &tab[2 * i], &tab[2 * i + 1]);
        SSW_TRY(grow_as(ctx->locate.angle_tab, tab.size() * sizeof(int32_t), dev_tab));
        SSW_TRY(upload(ctx, dev_tab, tab.data(), tab.size() * sizeof(int32_t), st));
        untimed_work(ctx);
        size_t bytes = 0;
        const auto take = [&bytes](size_t b) { const size_t at = bytes; bytes += b; return at; };
        const size_t word = sizeof(unsigned long long);
        const size_t o_res = take(n * 3 * word), o_rungs = take(n * 2 * n_rungs * word), o_fine = take(n * 2 * ANGLE_SLOTS * word);
        const size_t o_kept = take(report ? n * word : 0);
        zeroed = bytes;
        const size_t o_slots = take(n * ANGLE_SLOTS * sizeof(int32_t)), o_groups = take(report ? n * sizeof(ShareGroup) : 0);
        const size_t o_cands = take(report ? n * ANGLE_SLOTS * sizeof(ShareCand) : 0);
        uint8_t* base = nullptr;
        SSW_TRY(grow_as(ctx->locate.angle_sums, bytes, base));
        using Sums = unsigned long long*;
        res = reinterpret_cast<Sums>(base + o_res); rungs = reinterpret_cast<Sums>(base + o_rungs); fine = reinterpret_cast<Sums>(base + o_fine);
        kept = reinterpret_cast<Sums>(base + o_kept); slots = reinterpret_cast<int32_t*>(base + o_slots);
        groups = reinterpret_cast<ShareGroup*>(base + o_groups); cands = reinterpret_cast<ShareCand*>(base + o_cands);
        per = std::min(n, std::min(ANG_GROUP_MAX, std::max<size_t>(1, ANG_GROUP_BYTES / (extra + sl + sq))));
        SSW_TRY(grow_as(ctx->locate.luma, (size_t)lp * h + 16, lo));
        SSW_TRY(grow_as(ctx->locate.phases, (size_t)qp * hq + 16, lo4));
        SSW_TRY(grow_as(ctx->locate.group, per * (sl + sq) + 16, sus_l));
        sus_q = sus_l + per * sl;
        return SSW_OK;
    }
    // the sums zeroed and the original's luma and 4 x 4 box planes
    int original_planes(const uint8_t* dev_base) {
        SSW_HIP_CHECK(hipMemsetAsync(res, 0, zeroed, ctx->stream));
        SSW_TRY(locate_luma_planes(ctx, dev_base, 1, w, h, lo, 0, lp));
        return locate_box4_planes(ctx, lo, 0, lp, 1, w, h, lo4, 0, qp);
    }
    // ... and those of the m suspects of a group
    int suspect_planes(const uint8_t* frames, size_t m) {
        SSW_TRY(locate_luma_planes(ctx, frames, m, w, h, sus_l, sl, lp));
        return locate_box4_planes(ctx, sus_l, sl, lp, m, w, h, sus_q, sq, qp);
    }
    // a level for the group that begins at suspect g0: the ladder, every rung at f = 4 on the box planes, or the refinement, the
    // slot lists at f = 1 on the luma planes
    AngleLevel level(bool refine, size_t g0) const {
        AngleLevel lv{};
        lv.tab = dev_tab; lv.a_lo = a_lo; lv.a_first = a_lo; lv.w = (uint32_t)w; lv.h = (uint32_t)h; lv.ps_stride = refine ? sl : sq;
        lv.po = refine ? lo : lo4; lv.ps = refine ? sus_l : sus_q; lv.po_pitch = lv.ps_pitch = refine ? lp : qp;
        lv.wr = (uint32_t)(refine ? w : wq); lv.hr = (uint32_t)(refine ? h : hq); lv.f = refine ? 1 : 4; lv.sh = refine ? 17 : 19;
        lv.tiles_x = (lv.wr + TURN_TILE_W - 1) / TURN_TILE_W; lv.n_slots = refine ? ANGLE_SLOTS : n_rungs;
        lv.sums = refine ? fine + g0 * 2 * ANGLE_SLOTS : rungs + g0 * 2 * n_rungs;
        return lv;
    }
    // the ladder's launch of m suspects, nested as the coarse pass, as ssw_locate_rgb8 bills its own; then their kept rungs' slot lists
    template <class Launch> int ladder(size_t g0, size_t m, Launch launch) {
        {
            StageTimer tc(ctx, SSW_STAGE_LOCATE_COARSE, ctx->stream);
            if (ctx->timing) ctx->stage_work[SSW_STAGE_LOCATE_COARSE] += (double)m * n_rungs * pq;       // byte differences, not bytes
            SSW_TRY(launch());
        }
        angle_keep_kernel<<<(unsigned)m, 256, 0, ctx->stream>>>(rungs + g0 * 2 * n_rungs, n_rungs, j0, j1, slots + g0 * ANGLE_SLOTS);
        SSW_HIP_CHECK(hipGetLastError());
        return SSW_OK;
    }
    // the answers of m suspects from their refinement sums
    int answers(size_t g0, size_t m) {
        angle_final_kernel<<<(unsigned)((m + 63) / 64), 64, 0, ctx->stream>>>(slots + g0 * ANGLE_SLOTS, fine + g0 * 2 * ANGLE_SLOTS, (unsigned)m, res + 3 * g0);
        SSW_HIP_CHECK(hipGetLastError());
        return SSW_OK;
    }
    ssw_angle_found found(const uint64_t* got) const { return ssw_angle_found{(int32_t)(int64_t)got[0], n_rungs, got[1], got[2]}; }
};
static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the sums come down as they are");

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
    AngleSearch s(ctx, n, w, h, j0, j1);
    SSW_TRY(s.init(0, false));
    const unsigned n_rungs = s.n_rungs;
    {
        // plane bytes: made once, read once per candidate
        StageTimer t(ctx, SSW_STAGE_LOCATE, st, (double)(n + 1) * (4.0 * s.px + 2.0 * s.pq) + (double)n * 2.0 * (n_rungs * s.pq + ANGLE_SLOTS * s.px));
        SSW_TRY(s.original_planes(dev_base));
        for (size_t g0 = 0; g0 < n; g0 += s.per) {
            const size_t m = std::min(s.per, n - g0);
            SSW_TRY(s.suspect_planes(dev_suspects + g0 * w * h * 3, m));
            const AngleCost rung{s.level(false, g0), nullptr};
            SSW_TRY(s.ladder(g0, m, [&] { return angle_launch(ctx, rung, m); }));
            untimed_work(ctx);                                          // (the call's own timer ends behind everything, not with the ladder's)
            SSW_TRY(angle_launch(ctx, AngleCost{s.level(true, g0), s.slots + g0 * ANGLE_SLOTS}, m));
            SSW_TRY(s.answers(g0, m));
        }
    }
    std::vector<uint64_t> got(n * (3 + 2 * (size_t)n_rungs));           // the answers and the rung sums lie together
    SSW_HIP_CHECK(hipMemcpyAsync(got.data(), s.res, got.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    untimed_work(ctx);
    SSW_HIP_CHECK(hipStreamSynchronize(st));
    for (size_t i = 0; i < n; ++i) host_found[i] = s.found(&got[3 * i]);
    if (host_rungs) std::copy(got.begin() + 3 * n, got.end(), host_rungs);
    return SSW_OK;
}

// ---- the unknown-angle row of the strength report ----------------------------------------------------------------------------
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
    // a group: the turned frames and their planes, ANG_GROUP_BYTES at most
    AngleSearch s(ctx, N, w, h, j0, j1);
    SSW_TRY(s.init(fb, true));
    const unsigned n_rungs = s.n_rungs;
    const size_t per = s.per;
    const double px = s.px, pq = s.pq;
    uint8_t* turned_ws = nullptr;
    if (!dev_turned) SSW_TRY(grow_as(ctx->shared.affine, per * fb, turned_ws));
    {
        StageTimer t(ctx, SSW_STAGE_LOCATE, st, 4.0 * px + 2.0 * pq);
        SSW_TRY(s.original_planes(dev_base));
    }
    std::map<int32_t, size_t> kept_at;                       // the angle found -> where its mask is counted
    std::vector<int32_t> found_n(N);
    std::vector<int32_t> host_slots;
    std::vector<uint64_t> got;
    std::vector<ShareCand> cands;
    for (size_t g0 = 0; g0 < N; g0 += per) {
        const size_t m = std::min(per, N - g0);
        uint8_t* T = dev_turned ? dev_turned + g0 * fb : turned_ws;
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
        SSW_TRY(upload(ctx, s.groups, groups.data(), groups.size() * sizeof(ShareGroup), st));
        untimed_work(ctx);
        {
            // the ladder: every member of a share-group
            StageTimer t(ctx, SSW_STAGE_LOCATE, st, (double)m * (4.0 * px + 2.0 * pq + 2.0 * n_rungs * pq));
            SSW_TRY(s.suspect_planes(T, m));
            const AngleShared rung{s.level(false, g0), s.groups, nullptr, 0};
            SSW_TRY(s.ladder(g0, m, [&] { return angle_shared_launch(ctx, rung, n_rungs, (unsigned)groups.size()); }));
        }
        // the first wait of the group: the slot lists come down, the host forms the unions and who wants what
        host_slots.resize(m * ANGLE_SLOTS);
        SSW_TRY(download(ctx, host_slots.data(), s.slots + g0 * ANGLE_SLOTS, m * ANGLE_SLOTS * sizeof(int32_t), st));
        angle_share_cands(host_slots.data(), groups, cands);
        SSW_TRY(upload(ctx, s.groups, groups.data(), groups.size() * sizeof(ShareGroup), st));
        SSW_TRY(upload(ctx, s.cands, cands.data(), cands.size() * sizeof(ShareCand), st));
        untimed_work(ctx);
        {
            // the refinement: one launch per share-group, its grid exactly the group's candidates
            StageTimer t(ctx, SSW_STAGE_LOCATE, st, (double)cands.size() * px + (double)m * ANGLE_SLOTS * px);
            AngleShared d{s.level(true, g0), s.groups, s.cands, 0};
            for (size_t sg = 0; sg < groups.size(); ++sg) {
                if (!groups[sg].n_cands) continue;
                d.sg0 = (uint32_t)sg;
                SSW_TRY(angle_shared_launch(ctx, d, groups[sg].n_cands, 1));
            }
            SSW_TRY(s.answers(g0, m));
        }
        // the second wait: the answers, which shape the undoing
        got.resize(3 * m);
        SSW_TRY(download(ctx, got.data(), s.res + 3 * g0, 3 * m * sizeof(uint64_t), st));
        untimed_work(ctx);
        for (size_t i = 0; i < m; ++i) {
            host_found[g0 + i] = s.found(&got[3 * i]);
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
                        SSW_TRY(affine_kept_enqueue(ctx, w, h, B, F, s.kept + at));
                    }
                }
                i0 = i1;
            }
        }
    }
    // the call's last wait: the rung sums and the masks' counts
    std::vector<uint64_t> counts(kept_at.size());
    if (!counts.empty()) SSW_HIP_CHECK(hipMemcpyAsync(counts.data(), s.kept, counts.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    if (host_rungs) SSW_HIP_CHECK(hipMemcpyAsync(host_rungs, s.rungs, N * 2 * (size_t)n_rungs * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    untimed_work(ctx);
    SSW_HIP_CHECK(hipStreamSynchronize(st));
    for (size_t i = 0; i < N; ++i) {
        const auto it = kept_at.find(found_n[i]);
        host_kept[i] = it == kept_at.end() ? (uint64_t)w * h : counts[it->second];
    }
    return SSW_OK;
}
