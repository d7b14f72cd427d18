// The operand-ready f64 GEMM kernel (template) shared by its two translation units: dct_pair_f64.hip (forward instances,
// launch logic) and dct_pair_f64_inv.hip (inverse instances) -- one unit took six minutes to compile.
#pragma once
// Operand-ready even/odd-folded basis GEMMs in f64 (canonical precision).
//
// Measured on MI355X (tools/mfma_peak.hip): v_mfma_f64_16x16x4_f64 sustains 77.6 TFLOP/s when the
// wave issues nothing else, but every VALU instruction issued next to it takes MFMA pipe time --
// ~6 cycles for a 32-bit op, ~11.5 cycles for v_cvt_f64_f32 / v_add_f64 -- even from another wave
// of the same SIMD: one f64 VALU op per MFMA costs 16 % of the pipe.
//
// Here the GEMM main loop is DMA -> ds_read -> MFMA with scalar k-offsets: no VALU instruction except four address adds
// per k-step.  Its operands are produced once per pass by HBM-bound pre-passes (dct_pair_prep.hip) in exactly the form the
// MFMA consumes:
//   forward:  S[s] = (double)x[s] + (double)x[N-1-s],  D[s] = (double)x[s] - (double)x[N-1-s]
//   inverse:  E[s] = (double)c[2s],                    O[s] = (double)c[2s+1]
// stored k-blocked: [Kp / 8][lines][8] doubles (zero padded to Kp), i.e. the 64-byte piece of every
// line that one k-step needs lies next to its neighbours' -- a block tile's k-step is ONE contiguous
// 8 KB read (whole 128-byte lines, one DRAM page) instead of 128 pieces 15 KB apart.  The half bases
// are cached in the same layout.  For the column pass the pre-pass also transposes, so that one
// "NT" kernel serves all four passes:
//   acc1[x][y] = sum_k X1[x][k] Y1[y][k],   acc2[x][y] = sum_k X2[x][k] Y2[y][k]
// with X = image operand (lines), Y = half basis (pairs).  Epilogues:
// forward interleaves (even, odd) frequencies; inverse forms acc1 +/- acc2 for the mirrored
// positions; results are rounded once to f32 (then the reference's f32 scale factor, if any).
//
// The odd halves are split once more (dct_pair_prep.hip, "Split odd half"): their launches feed this kernel two
// DIFFERENT image operands (the rotated and folded AS | BD or AD | BS) against quarter-length cosine / sine bases and
// the epilogues emit acc1 +/- acc2 (po.pm); a deep inverse adds EPI_INV_OT (the half-length even half E from its own
// even half T2 and odd part).  Row passes store through buffer instructions with per-tile lane offsets (epilogue notes
// below); deep transforms keep the plane between their passes class-major (dct_pair_common.hpp).  What a launch class
// is -- pairs, sum length, output map, template instance -- is one row of the table in dct_pair_class.hpp.
//
// Block: 256 threads = 4 waves as 2 x 2; block tile 128 lines x 64 pairs x 2 products; k-step 8;
// per wave 16 MFMA 16x16 tiles = 128 accumulator registers; 2 blocks per CU.  The operand tiles arrive by LDS-DMA
// (buffer_load ... lds, 16 bytes per lane) in a ring of two 24-KB stages [X1 | X2 | Y1 | Y2] = 48 KB of LDS, one k-step
// ahead of the MFMAs; the swizzle sits on the lanes' source addresses (chunk c of tile row r lands at c ^ ((r >> 2) & 3):
// conflict-free ds_read_b64 fragment reads).  In the middle of k-step t a wave waits for its own DMA of stage t + 1 and its
// last fragment reads of stage t, passes one raw s_barrier, and re-requests stage t for k-step t + 2; any number of
// k-steps >= 2.
// Lane l: li = l & 15 (line / pair inside a 16x16 tile), lq = l >> 4: in half-step s lane group lq
// supplies k = 4 s + lq (the same assignment on both operands).
#include "dct_pair_common.hpp"
#include "dct_pair_colops.hpp"

#include <cstdlib>
#include <type_traits>


namespace ssw {

constexpr int PT = 256;
constexpr int PBK = 8;
constexpr int RGB_NB = 2;      // output rows whose I / Q quads the RGB epilogue keeps in flight together (4: a spill in the loop at 256 VGPRs)

#ifdef SSW_TILE_TRACE
// diagnostic build only (tools/tile_trace.py): the trace globals are defined by dct_pair_f64.hip before this header
#define SSW_TT(i) do { if (threadIdx.x == 0) tt[i] = wall_clock64(); } while (0)
// ... and per k-step (the barrier in the middle of step t has been passed): 32-bit wall-clock stamps of up to 32 steps per tile
// (into LDS: a global store -- and the load of the trace pointer -- inside the loop made the compiler drain the loop's prefetch
// with vmcnt(0) at every step and doubled the main loop; trace_end copies them out)
#define SSW_KT(t) do { if (threadIdx.x == 0 && (t) < 32u) kst_lds[t] = (unsigned)wall_clock64(); } while (0)
#else
#define SSW_TT(i) do { } while (0)
#define SSW_KT(t) do { } while (0)
#endif
typedef PairOutT<double> PairOut;


// COLS: lines are (frame, column) and the transformed axis runs down the rows.  SAMEX: X2 == X1
// (one product's image operand feeds both basis operands; it is staged and read once).
// (A 256-line x 32-pair block tile for pair counts that 64 divides badly -- 540 at 4K -- was measured:
// equal on the shared-X launches, 10 % slower on the two-operand ones; not kept.)
// SUB only names the instance (launches that serve a deeper folding level show up separately in profiles).
// BM: lines per block tile.  128 is the tile of every large launch; 64 serves launches whose 128-line grid
// would leave the chip half empty (a single 4K frame: 17 x 15 = 255 tiles for 512 block slots).
// One launch serves up to eight "classes" (dct_pair_class.hpp) -- GEMMs of the same template instance over the same lines with their own
// operands, bases, pair counts, sum lengths and output maps: the tile columns of the classes lie side by side in the
// launch's tile grid.  Batch launches carry one class; the five launches of a deep forward pass (two or three of an
// inverse pass) of a single frame are merged into one, because each alone fills half of the chip's block slots for one
// round (a 4K frame's class E: 34 x 8 = 272 blocks of 64 lines for 512 slots).
struct PairMulti {
    PairClassArgs c[8];
    unsigned n_classes, L, tiles_m, tiles_n_total;
    PairOut po;                        // the fields the classes share; c1 .. bn32 are overwritten per class
    // forward column launches of a pruned base reader (BasePart::Phase1Cols / Phase2Cols): line tile tm = frame * need_tpf + column tile
    const unsigned* need = nullptr;
    unsigned need_mode = 0, need_tpf = 1;
    // gated tail row launches of a pruned base reader (SUB 5, BasePart::TailRows): `need` as above with need_tpf = column
    // tiles per frame; tail[0] counts the (frame, class, tile column) jobs that ran, tail[1] / tail[2] (doubles) their flop and
    // bytes at tail_flop / tail_bytes per pair of a job
    unsigned long long* tail = nullptr;
    double tail_flop = 0.0, tail_bytes = 0.0;
};

template <bool COLS, int EPI, bool SAMEX, int SUB = 0, int BM = 128>
__global__ __launch_bounds__(PT, 2) void pair_gemm_f64_kernel(const PairMulti ml, Epilogue ep) {
// (the host pass never generates code for a kernel body, but it does check it: the LDS-DMA builtins and the s_waitcnt statements
// made it drop the kernels' launch stubs without a word -- it sees an empty body)
#if defined(__HIP_DEVICE_COMPILE__)
    constexpr int NX = SAMEX ? 1 : 2;
    constexpr int BN = 64, XQ = BM / 64;                                   // XQ: X lines per staging thread
    // r6: the operand tiles arrive by LDS-DMA (buffer_load ... lds) in a ring of two stages [X1 | X2 | Y1 | Y2], one k-step ahead
    // of the MFMAs; a column pass reuses the region to transpose its results (epilogue)
    constexpr int STG = NX * BM * PBK + 2 * BN * PBK;                      // doubles per stage
    constexpr int SXD = 2 * STG;
    constexpr int TRD = COLS ? 4 * 32 * (BM / 2 + 16) / 2 : 0;              // 4 waves x 32 result rows x pitch floats
#ifdef SSW_TILE_TRACE
    __shared__ __attribute__((aligned(16))) double lds[(SXD > TRD ? SXD : TRD) + 16];
    unsigned* kst_lds = reinterpret_cast<unsigned*>(lds + (SXD > TRD ? SXD : TRD));
#else
    __shared__ __attribute__((aligned(16))) double lds[SXD > TRD ? SXD : TRD];
#endif

#ifdef SSW_TILE_TRACE
    unsigned long long tt[5] = {0, 0, 0, 0, 0};
    const unsigned long long cyc0 = clock64();
    unsigned kslot = 0xFFFFFFFFu;
    if (threadIdx.x == 0 && g_tile_trace) kslot = atomicAdd(&g_tile_trace_n, 1u);
#endif
    SSW_TT(0);
    unsigned tm, tn, cls = 0;
    tile_of_block(blockIdx.x, gridDim.x, ml.tiles_m, ml.tiles_n_total, tm, tn);
    while (cls + 1 < ml.n_classes && tn >= ml.c[cls].tiles_n) { tn -= ml.c[cls].tiles_n; ++cls; }      // block-uniform
    if constexpr (COLS && EPI == EPI_FWD && BM == 128 && SUB >= 10) {
        // pruned base reader (its own instance, SUB 13: every other column launch is the kernel it was).  Phase 1 computes column
        // tile 0 of every frame: its grid has one line tile per frame (ml.tiles_m = frames).  Phase 2 runs over every line tile
        // and computes the other tiles that are needed; a block of any other tile returns before it has issued a load (tm is
        // block-uniform: the flag is a scalar load)
        if (ml.need_mode == 1) tm *= ml.need_tpf;
        else if (tm % ml.need_tpf == 0 || ml.need[tm] == 0) return;
    }
    if constexpr (!COLS && EPI == EPI_FWD_COLOP && SUB == 5) {
        // tail row launches of a pruned base reader (their own instance, SUB 5): the class's tile columns from tn0 on.  A line
        // tile lies inside one frame z (unit-ordered, padded lines); the tile column's pairs write the column-operand lines of
        // the column tiles lo .. hi (entry e of a class -> tile e >> gsh; the second outputs of a class of E's shape lie one
        // entry lower).  A block returns before it has issued a load unless the decide kernel flagged one of them: the flags
        // are scalar loads, the branch is block-uniform.
        const PairClassArgs& cg = ml.c[cls];
        tn += cg.tn0;
        const unsigned tw = cg.bn32 == 2 ? 48u : 64u;
        const unsigned tpf = ml.po.cop_hup / 8, z = tm / tpf;
        const unsigned pf = tn * tw, pl = pf + tw - 1u < cg.NP ? pf + tw - 1u : cg.NP - 1u;
        const unsigned lo = (pf - cg.e2off) >> cg.gsh, hi = pl >> cg.gsh;
        unsigned any = 0;
        for (unsigned t = lo; t <= hi; ++t) any |= ml.need[(size_t)z * ml.need_tpf + t];
        if (!any) return;
        if (ml.tail && tm == z * tpf && threadIdx.x == 0) {
            const double pairs = (double)(pl - pf + 1u);
            atomicAdd(&ml.tail[0], 1ull);
            atomicAdd(reinterpret_cast<double*>(ml.tail) + 1, pairs * ml.tail_flop);
            atomicAdd(reinterpret_cast<double*>(ml.tail) + 2, pairs * ml.tail_bytes);
        }
    }
    const PairClassArgs& ca = ml.c[cls];
    const double* __restrict__ X1g = ca.x1;
    const double* __restrict__ X2g = ca.x2;
    const double* __restrict__ Y1g = ca.y1;
    const double* __restrict__ Y2g = ca.y2;
    const unsigned L = ml.L, NP = ca.NP, Kp = ca.Kp, yrows = ca.yrows;
    PairOut po = ml.po;
    po.c1 = ca.c1; po.c2 = ca.c2; po.cs = ca.cs; po.pm = ca.pm; po.np1 = ca.np1; po.p2lo = ca.p2lo; po.bn32 = ca.bn32; po.fold0 = ca.fold0;
    po.gsh = ca.gsh; po.e2off = ca.e2off;
    const unsigned m0 = tm * BM, p0 = tn * (po.bn32 == 1 ? 32u : po.bn32 == 2 ? 48u : (unsigned)BN);      // bn32: tile width code (PairOutT)
    const unsigned tid = threadIdx.x;
    const unsigned lane = tid & 63, wave = tid >> 6;
    const unsigned li = lane & 15, lq = lane >> 4;

    // LDS tile rows hold 8 consecutive k (64 bytes) as four 16-byte chunks; chunk c of row r sits at position c ^ ((r >> 2) & 3):
    // a wave's DMA instruction fills 16 consecutive rows (1 KB, lane l -> row l / 4, position l % 4: the LDS side of an LDS-DMA
    // is lane-linear, the swizzle is applied to the lane's SOURCE address), and the fragment reads (ds_read_b64: 16 rows x one
    // chunk per lane group) are conflict-free -- rows r, r + 4, r + 8, r + 12 share their banks and differ in (r >> 2) & 3.
    const unsigned wv = (unsigned)__builtin_amdgcn_readfirstlane((int)wave);
    const unsigned drow = 16 * wave + (lane >> 2), dch = lane & 3;       // row inside a 64-row piece group, position
    unsigned xoff[XQ];
#pragma unroll
    for (int q = 0; q < XQ; ++q) {
        // (column pass behind a fused row pass: the tile's lines are in class-major order, row j of the tile is line
        // fwd_cm128_pos(j) -- a permutation inside the same contiguous 8 KB of a k-step, whole 128-line tiles only)
        const unsigned j = drow + 64 * q;
        unsigned r = m0 + ((COLS && BM == 128 && po.xperm) ? fwd_cm128_pos(j) : j);
        r = r < L ? r : L - 1;
        xoff[q] = (r - m0) * 64u + 16u * (dch ^ ((j >> 2) & 3u));
    }
    unsigned yr = p0 + drow;
    yr = yr < NP ? yr : NP - 1;
    const unsigned yoff = (yr - p0) * 64u + 16u * (dch ^ ((drow >> 2) & 3u));
    // block-uniform buffer resources (scalar registers) at the tile's first line of k-block 0; a k-step
    // advances a scalar byte offset by one k-block (< 4 GB: checked by the launcher)
#ifdef SSW_ABL_X0          // timing-only ablation: every block stages the lines of tile 0 (L2-resident): what the operands' memory latency costs
    const size_t m0x = 0;
#else
    const size_t m0x = m0;
#endif
    const __amdgpu_buffer_rsrc_t x1r = __builtin_amdgcn_make_buffer_rsrc((void*)(X1g + m0x * 8), 0, 0xFFFFFFFFu, 0x00020000);
    const __amdgpu_buffer_rsrc_t x2r = __builtin_amdgcn_make_buffer_rsrc((void*)(X2g + m0x * 8), 0, 0xFFFFFFFFu, 0x00020000);
    const __amdgpu_buffer_rsrc_t y1r = __builtin_amdgcn_make_buffer_rsrc((void*)(Y1g + (size_t)p0 * 8), 0, 0xFFFFFFFFu, 0x00020000);
    const __amdgpu_buffer_rsrc_t y2r = __builtin_amdgcn_make_buffer_rsrc((void*)(Y2g + (size_t)p0 * 8), 0, 0xFFFFFFFFu, 0x00020000);
    const unsigned xstep = L * 64u, ystep = yrows * 64u;

    constexpr int LPT = XQ * NX + 2;                                   // DMA instructions per wave and stage
    typedef __attribute__((address_space(3))) void* lds_ptr_t;
    // stage `sb` (offset in doubles) <- k-step t
    auto issue = [&](unsigned t, unsigned sb) {
        const unsigned xadv = t * xstep, yadv = t * ystep;
        double* b = lds + sb + 16 * wv * PBK;
#pragma unroll
        for (int q = 0; q < XQ; ++q) {
            __builtin_amdgcn_raw_ptr_buffer_load_lds(x1r, (lds_ptr_t)(b + 64 * q * PBK), 16, xoff[q], xadv, 0, 0);
            if (!SAMEX) __builtin_amdgcn_raw_ptr_buffer_load_lds(x2r, (lds_ptr_t)(b + BM * PBK + 64 * q * PBK), 16, xoff[q], xadv, 0, 0);
        }
        __builtin_amdgcn_raw_ptr_buffer_load_lds(y1r, (lds_ptr_t)(b + NX * BM * PBK), 16, yoff, yadv, 0, 0);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(y2r, (lds_ptr_t)(b + NX * BM * PBK + BN * PBK), 16, yoff, yadv, 0, 0);
    };
    // The wave grid is 2 x 2 (each wave BM/2 lines x 32 pairs: NI = BM/32 line tiles) unless the tile holds at
    // most 32 valid pairs -- the last tile column of e.g. 540 pairs -- where it is 4 x 1 (each wave
    // BM/4 lines x 32 pairs: NI = BM/64) and the tile takes half the MFMAs instead of computing padding.
    auto run = [&](auto nic, auto njc) {
    constexpr int NI = decltype(nic)::value;
    constexpr int NJ = decltype(njc)::value;                 // pair tiles of 16 per wave: 2; 1 / 3 (4 x 1 grid) when the tile holds <= 16 / 33 .. 48 valid pairs
    constexpr int NJA = NJ < 2 ? 2 : NJ;
    constexpr bool FULL = NI == BM / 32;
    const unsigned wm = FULL ? (wave >> 1) * (BM / 2) : wave * (BM / 4), wn = FULL ? (wave & 1) * 32 : 0;
    f64x4 acc1[NI][NJA], acc2[NI][NJA];
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = 0; j < NJA; ++j) { acc1[i][j] = (f64x4){0, 0, 0, 0}; acc2[i][j] = (f64x4){0, 0, 0, 0}; }

    // fragment of half-step s: lane group lq supplies k = 4 s + lq, i.e. half lq & 1 of chunk 2 s + lq / 2 (position: chunk ^ swizzle
    // of the row; wm, wn and the 16-row tile offsets are multiples of 16, so the swizzle depends on li alone)
    const unsigned fsw = (li >> 2) & 3;
    unsigned rdx[2], rdy[2];
#pragma unroll
    for (int sh = 0; sh < 2; ++sh) {
        rdx[sh] = (wm + li) * PBK + 2 * ((2 * sh + (lq >> 1)) ^ fsw) + (lq & 1);
        rdy[sh] = NX * BM * PBK + (wn + li) * PBK + 2 * ((2 * sh + (lq >> 1)) ^ fsw) + (lq & 1);
    }
    struct Frag { double x1[NI], x2[NI], y1[NJA], y2[NJA]; };
    auto fread = [&](unsigned sb, auto shc, Frag& f) {
        constexpr int sh = decltype(shc)::value;
        const double* b = lds + sb;
#pragma unroll
        for (int jn = 0; jn < NJ; ++jn) {
            f.y1[jn] = b[rdy[sh] + 16 * jn * PBK];
            f.y2[jn] = b[rdy[sh] + BN * PBK + 16 * jn * PBK];
        }
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            f.x1[i] = b[rdx[sh] + 16 * i * PBK];
            if (!SAMEX) f.x2[i] = b[rdx[sh] + BM * PBK + 16 * i * PBK];
        }
    };
    auto fmma = [&](const Frag& f) {
#pragma unroll
        for (int i = 0; i < NI; ++i)
#pragma unroll
            for (int jn = 0; jn < NJ; ++jn) {
                const double xb = SAMEX ? f.x1[i] : f.x2[i];
                if (!COLS) {      // D[row = line][col = pair]
                    acc1[i][jn] = __builtin_amdgcn_mfma_f64_16x16x4f64(f.x1[i], f.y1[jn], acc1[i][jn], 0, 0, 0);
                    acc2[i][jn] = __builtin_amdgcn_mfma_f64_16x16x4f64(xb, f.y2[jn], acc2[i][jn], 0, 0, 0);
                } else {          // D[row = pair][col = line]: image columns along the lanes
                    acc1[i][jn] = __builtin_amdgcn_mfma_f64_16x16x4f64(f.y1[jn], f.x1[i], acc1[i][jn], 0, 0, 0);
                    acc2[i][jn] = __builtin_amdgcn_mfma_f64_16x16x4f64(f.y2[jn], xb, acc2[i][jn], 0, 0, 0);
                }
            }
    };
    using B0 = std::integral_constant<int, 0>;
    using B1 = std::integral_constant<int, 1>;
    // One LDS read behind each of the first MFMAs of a half-step, then (second half) one DMA instruction behind each of the next
    auto interleave = [&](auto dmac) {
        constexpr int NDMA = decltype(dmac)::value;
        constexpr int NMF = 2 * NJ * NI;                        // MFMAs per half-step
        constexpr int NRD = (2 * NJ + NI * NX + 1) / 2;         // ds_read2_b64 per half-step (fragments pair up)
#pragma unroll
        for (int i = 0; i < NRD; ++i) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        }
#pragma unroll
        for (int i = 0; i < NDMA; ++i) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
        }
        __builtin_amdgcn_sched_group_barrier(0x008, NMF - NRD - NDMA > 0 ? NMF - NRD - NDMA : 0, 0);
        __builtin_amdgcn_sched_barrier(0);
    };
    // The ring.  Stage t % 2 holds k-step t; the barrier in the middle of step t is passed when every wave's DMA of stage t + 1 has
    // landed (each wave waits for its own: vmcnt(0), nothing else is in flight then) and when every wave has its last fragments
    // of stage t in registers (lgkmcnt(0)): stage t is refilled with k-step t + 2 right behind the barrier, one k-step before its
    // first read, while the MFMAs of stage t + 1 run.
    const unsigned nk = Kp / PBK;          // >= 2
    Frag fa, fb;
    issue(0, 0);
    issue(1, STG);
    asm volatile("s_waitcnt vmcnt(%0)" :: "n"(LPT) : "memory");
    asm volatile("s_barrier" ::: "memory");
    SSW_TT(1);
    fread(0u, B0{}, fa);
    unsigned cur = 0, nxt = STG, t = 0;
    // one k-step: second half-step of stage `cur`, the barrier, first half-step of stage `nxt`.  ISSUE: k-step t + 2 exists and is
    // requested into stage `cur`
    auto step = [&](auto issuec) {
        constexpr bool ISSUE = decltype(issuec)::value != 0;
        fread(cur, B1{}, fb);
        fmma(fa);
        interleave(B0{});
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
        SSW_KT(t);
        fread(nxt, B0{}, fa);
        if (ISSUE) issue(t + 2, cur);          // (behind the reads in program order: LDS accesses keep theirs, so the DMA instructions can then go one per MFMA)
        fmma(fb);
        interleave(std::integral_constant<int, ISSUE ? LPT : 0>{});
        cur = nxt;
        nxt = nxt + STG == 2 * STG ? 0u : nxt + STG;
        ++t;
    };
    while (t + 2 < nk) step(B1{});
    if (t + 1 < nk) step(B0{});                // k-step nk - 2: the last stage must have landed
    fread(cur, B1{}, fb);
    fmma(fa);
    interleave(B0{});
    fmma(fb);
    SSW_TT(2);
#ifdef SSW_ABL_NOEPI       // timing-only ablation: no epilogue (one store keeps the accumulators alive)
    if (acc1[0][0][0] + acc2[NI - 1][NJ - 1][3] == 1.2345e300) po.out[0] = 1.f;
    return;
#endif

#ifdef SSW_TILE_TRACE
    auto trace_end = [&]() {
    __builtin_amdgcn_sched_barrier(0);
    if (threadIdx.x == 0) tt[4] = wall_clock64();
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_waitcnt(0);
    if (threadIdx.x == 0 && g_tile_trace) {
        tt[3] = wall_clock64();
        const unsigned slot = kslot;
        if (slot < g_tile_trace_cap) {
            unsigned hwid = 0, xcc = 0;
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
            unsigned long long* o = g_tile_trace + 8ull * slot;
            o[0] = tt[0]; o[1] = tt[1]; o[2] = tt[2]; o[3] = tt[3];
            o[4] = ((unsigned long long)xcc << 32) | hwid;
            o[5] = (unsigned long long)(unsigned)(COLS * 1000 + EPI * 100 + SAMEX * 10 + SUB);
            o[6] = ((unsigned long long)Kp << 32) | NP;
            o[5] |= ((clock64() - cyc0) & 0xFFFFFFFull) << 36;     // shader cycles of the block (28 bits) above the tag
            o[7] = tt[4];
            if (g_tile_kstep)
                for (unsigned i = 0; i < 32u; ++i) g_tile_kstep[32ull * slot + i] = kst_lds[i];
        }
    }
    };
#else
    auto trace_end = [] {};
#endif
    if (po.pm) {                               // split odd half: cosine part +/- sine part (block-uniform branch)
        // fold0 (class E): pair 0 multiplied cosine row 0 and sine row n/8; its outputs are acc1 itself (first output of
        // pair 0: the sine row of pair 0 is zero) and -acc2 (second output of pair n/8: its cosine row is zero).  Only the
        // first tile column holds pair 0: block-uniform branch, one select per value there.
        const bool has0 = po.fold0 != 0 && p0 == 0 && wn == 0;
#pragma unroll
        for (int i = 0; i < NI; ++i)
#pragma unroll
            for (int jn = 0; jn < NJ; ++jn)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double a1 = acc1[i][jn][r], a2 = acc2[i][jn][r];
                    double s = a1 + a2, d = a1 - a2;
                    if (jn == 0 && has0) {
                        // !COLS: the pair runs along the lanes (li); COLS: along the accumulator rows (lq + 4 r)
                        const bool p = COLS ? (lq == 0 && r == 0) : (li == 0);
                        s = p ? a1 : s;
                        d = p ? 0.0 - a2 : d;
                    }
                    acc1[i][jn][r] = s;
                    acc2[i][jn][r] = d;
                }
    }
    const bool second_out = po.pm != 2;
    // pair whose second output this pair's slot carries (fold0: pair 0 carries pair n/8's)
    auto p2 = [&](unsigned pair) { return (po.fold0 && pair == 0) ? po.fold0 : pair; };

    // D map of 16x16x4 f64: col = lane & 15, row = (lane >> 4) + 4 reg
    const unsigned n = po.n, W = po.W, H = po.H;
    // one output line: element idx of the transformed axis lives at lp[idx * es] (and tp[idx * es] in T)
    // element offsets idx * es stay below 2^32 (W * H < 2^32: indices are u32 throughout)
    // position of element m of a line of length len: natural, or class-major on the row pass of a deep inverse transform
    auto opos = [&](unsigned m, unsigned len) { return (!COLS && po.cm) ? inverse_class_pos(m, len, 0, po.cm == 2) : m; };
    // ... of T2 as EPI_INV_OT reads it (length n/2): natural, or mod-4 class-major (po.tcm)
    auto tpos = [&](unsigned m) { return (!COLS && po.tcm) ? inverse_class_pos(m, n / 2, 0, false) : m; };
    // ... of the f32 output line (class-major inside tiles of po.cmt positions; the E planes above: one tile)
    auto oposf = [&](unsigned m, unsigned len) { return (!COLS && po.cm) ? inverse_class_pos(m, len, po.cmt, po.cm == 2) : m; };
    // forward outputs of a pair: natural c + cs pair, or the class-major column of its entry (PairOutT::ft)
    auto fpos1 = [&](unsigned pair) {
        return po.ft ? po.c1 + (pair >> po.gsh) * po.ft + (pair & ((1u << po.gsh) - 1u)) : po.c1 + po.cs * pair;
    };
    auto fpos2 = [&](unsigned pair) {
        const unsigned q = p2(pair), e = q - po.e2off;
        return po.ft ? po.c2 + (e >> po.gsh) * po.ft + (e & ((1u << po.gsh) - 1u)) : po.c2 + po.cs * q;
    };
    auto emit = [&](float* lp, double* tp, double* to, unsigned es, unsigned pair, double a1, double a2) {
        if (EPI == EPI_FWD || EPI == EPI_FWD_ADJ) {
            const unsigned i1 = fpos1(pair), i2 = fpos2(pair);
            if (EPI == EPI_FWD_ADJ) {
                const f32x2 v = {apply_epilogue(ep, (float)a1, i1), apply_epilogue(ep, (float)a2, i2)};
                *reinterpret_cast<f32x2*>(lp + i1) = v;
            } else {
                if (pair < po.np1) lp[i1 * es] = apply_epilogue(ep, (float)a1, i1);
                if (pair >= po.p2lo && second_out) lp[i2 * es] = apply_epilogue(ep, (float)a2, i2);
            }
        } else if (EPI == EPI_INV) {
            lp[pair * es] = apply_epilogue(ep, (float)(a1 + a2), pair);
            lp[(n - 1 - pair) * es] = apply_epilogue(ep, (float)(a1 - a2), n - 1 - pair);
        } else if (EPI == EPI_INV_E) {
            tp[pair * es] = a1 + a2;
            tp[(n / 2 - 1 - pair) * es] = a1 - a2;
        } else if (EPI == EPI_INV_OT) {
            const unsigned n1 = po.c1 + po.cs * pair, n2 = po.c2 + po.cs * p2(pair);
            if (n1 < n / 2) { const double e1 = tp[tpos(n1) * es]; to[opos(n1, n) * es] = e1 + a1; to[opos(n - 1 - n1, n) * es] = e1 - a1; }
            if (n2 < n / 2) { const double e2 = tp[tpos(n2) * es]; to[opos(n2, n) * es] = e2 + a2; to[opos(n - 1 - n2, n) * es] = e2 - a2; }
        } else {
            const unsigned n1 = po.c1 + po.cs * pair, n2 = po.c2 + po.cs * p2(pair);      // positions in the odd part, < n/2
            if (n1 < n / 2) {
                const double e1 = tp[opos(n1, n / 2) * es];
                lp[oposf(n1, n) * es] = apply_epilogue(ep, (float)(e1 + a1), n1);
                lp[oposf(n - 1 - n1, n) * es] = apply_epilogue(ep, (float)(e1 - a1), n - 1 - n1);
            }
            if (n2 < n / 2) {
                const double e2 = tp[opos(n2, n / 2) * es];
                lp[oposf(n2, n) * es] = apply_epilogue(ep, (float)(e2 + a2), n2);
                lp[oposf(n - 1 - n2, n) * es] = apply_epilogue(ep, (float)(e2 - a2), n - 1 - n2);
            }
        }
    };
    // r5: forward row pass whose results go straight into the COLUMN pass's operand planes (EPI_FWD_COLOP, see
    // dct_pair_common.hpp).  Tile tm = (frame z, unit group g): its 128 lines are the units 8 g .. 8 g + 7 of frame z, MFMA
    // line tile i of this wave is unit u0 + i, and the tile's pairs are 2 x 16 NJ frequencies ("items") per wave.
    //   1. per unit: every lane puts its 4 x 2 NJ results (rounded to f32 = the store between the passes,
    //      src/dct2d.rs:152-168; then the per-index f32 factor) into the wave's LDS area [item][line of the unit], pitch 20
    //      floats (conflict-free both ways), and reads back the sixteen lines of ITS item (lane, lane + 64);
    //   2. col_l2_unit (the column pre-pass's arithmetic, tables of the unit by scalar index) -> sixteen doubles per item and unit;
    //   3. per item and plane the NI units are NI consecutive doubles of one k-block piece: one or two 16-byte stores; the
    //      two waves that share a tile row complete the 64-byte pieces, the pairs of one MFMA tile complete runs of
    //      16 lines x 64 bytes per (plane, 128-frequency tile).
    if constexpr (!COLS && EPI == EPI_FWD_COLOP) {
        constexpr int NIT = 32 * NJ, NC = (NIT + 63) / 64;
        constexpr int NPT = FULL ? 64 : 16 * NJ, NLT = 2 * NPT;            // pairs / column-operand lines of the whole tile
        static_assert(4 * NIT * 16 * 4 <= (int)sizeof(lds) && 4 * NLT * 64 <= (int)sizeof(lds), "transpose area, store slabs");
        static_assert(BM == 128, "a tile is one k-block of eight units");
        __syncthreads();                      // every wave has read its last fragments: the operand tiles are free
        float* tw = reinterpret_cast<float*>(lds) + wave * (NIT * 16);
        auto lds_order = [&]() {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        };
        const unsigned Hc = po.H, HU = Hc / 16;
        const unsigned tpf = po.cop_hup / 8;                       // line tiles per frame
        const unsigned z = tm / tpf, g = tm - z * tpf;
        const unsigned u0 = (unsigned)__builtin_amdgcn_readfirstlane((int)(wm / 16));
        const bool plain = ep.first == 1.0f && ep.base == 1.0f;
        // LDS position of line v of item f in the wave's transpose area: 16 floats per item, the four quads of an item
        // XOR-swizzled by (item / 4) & 3 -- conflict-free for the ds_write_b32 of a lane group and the ds_read_b128 of 16 items
        auto lpos = [&](unsigned f, unsigned v) { return f * 16u + 4u * ((v >> 2) ^ ((f >> 2) & 3u)) + (v & 3u); };
        // f32 factor of the frequencies this lane's accumulators belong to (EPI_FWD: first for index 0, else base)
        float f1[NJ], f2[NJ];
#pragma unroll
        for (int jn = 0; jn < NJ; ++jn) {
            const unsigned pair = p0 + wn + 16 * jn + li;
            f1[jn] = fpos1(pair) == 0 ? ep.first : ep.base;
            f2[jn] = fpos2(pair) == 0 ? ep.first : ep.base;
        }
        // energy instances: sum of squares of this lane's f32 values per output, i.e. per column-operand line (f32 VALU only);
        // block totals of the tile's 64 pairs x 2 outputs in the 16 KB of LDS above the store slabs
        constexpr bool ENERGY = SUB >= 10;
        float en1[NJ], en2[NJ];
        float* eb = reinterpret_cast<float*>(lds + 4 * 128 * 8);
        if constexpr (ENERGY) {
            static_assert(4 * 128 * 64 + 128 * 4 <= (int)sizeof(lds), "energy totals above the slabs");
#pragma unroll
            for (int jn = 0; jn < NJ; ++jn) { en1[jn] = 0.f; en2[jn] = 0.f; }
            if (tid < 128) eb[tid] = 0.f;
        }
        // phase A: this lane's items (item f = lane + 64 c of the wave: pair tile f / 32, output (f / 16) & 1, pair f & 15),
        // all sixteen planes of the wave's NI units
        double o[NC][NI][16];
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            lds_order();
#pragma unroll
            for (int jn = 0; jn < NJ; ++jn)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float v1 = (float)acc1[i][jn][r], v2 = (float)acc2[i][jn][r];
                    if (!plain) { v1 *= f1[jn]; v2 *= f2[jn]; }
                    if constexpr (ENERGY) { en1[jn] = __builtin_fmaf(v1, v1, en1[jn]); en2[jn] = __builtin_fmaf(v2, v2, en2[jn]); }
                    tw[lpos(32 * jn + li, lq + 4 * r)] = v1;
                    tw[lpos(32 * jn + 16 + li, lq + 4 * r)] = v2;
                }
            lds_order();
            const unsigned e = (unsigned)__builtin_amdgcn_readfirstlane((int)(8 * g + u0 + i));
            const bool unit_ok = e < HU;
            const ColL2Tab tab = col_l2_tab(po.crot1, po.crot2, po.crot3, unit_ok ? e : 0u, Hc);
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const unsigned f = (lane + 64 * c) < (unsigned)NIT ? lane + 64 * c : 0u;
                float x[16];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const f32x4 t4 = *reinterpret_cast<const f32x4*>(tw + lpos(f, 4 * q));
                    x[4 * q] = t4[0]; x[4 * q + 1] = t4[1]; x[4 * q + 2] = t4[2]; x[4 * q + 3] = t4[3];
                }
                col_l2_unit(x, tab, o[c][i]);
                if (!unit_ok) {
#pragma unroll
                    for (int a = 0; a < 16; ++a) o[c][i][a] = 0.0;              // units beyond the axis: the planes' zero padding
                }
            }
        }
        // phase B: the results leave through LDS slabs that are images of the stored runs.  (Stored straight from the lanes --
        // 16 bytes of 64 different pieces per instruction -- every piece was a partial write that made the L2 fetch its line
        // first: PMC FETCH_SIZE of a launch 2.17 GB against 1.07 GB of operands, profiles/r5_pmc_traffic.json.)  Tile line
        // T = 16 (pair / 8) + 8 output + pair % 8 of the tile's pairs: eight pairs' first outputs and their second outputs
        // are sixteen consecutive column-operand lines (ForwardClassLayout: two neighbouring classes, eight entries per
        // 128-column tile).  A slab = one plane x the tile's 2 NPT lines x the k-block's eight units (64 bytes per line; the
        // four 16-byte chunks of a line XOR-swizzled by (T / 4) & 3); four planes per round, four rounds.  Store sweep: thread
        // = (line, chunk), four lanes complete a 64-byte piece, a wave writes 1 KB of sixteen consecutive lines.
        if constexpr (ENERGY) {
            __syncthreads();                  // the totals are zero
#pragma unroll
            for (int jn = 0; jn < NJ; ++jn) {
                float a = en1[jn], b = en2[jn];
                a += __shfl_xor(a, 16); a += __shfl_xor(a, 32);
                b += __shfl_xor(b, 16); b += __shfl_xor(b, 32);
                if (lq == 0) {
                    const unsigned pl = wn + 16 * jn + li;              // pair inside the tile
                    atomicAdd(eb + pl, a);
                    atomicAdd(eb + 64 + pl, b);
                }
            }
        }
        double* slab = lds;
        unsigned tl[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const unsigned f = lane + 64 * c, pl = wn + 16 * (f >> 5) + (f & 15u);      // pair inside the tile
            tl[c] = f < (unsigned)NIT ? 16u * (pl >> 3) + 8u * ((f >> 4) & 1u) + (pl & 7u) : 0u;
        }
        constexpr int NSW = (NLT * 4 + 255) / 256;                 // (line, chunk) items per thread of the store sweep
        bool st_ok[NSW];
        size_t st_off[NSW];
        unsigned st_lds[NSW];
#pragma unroll
        for (int j = 0; j < NSW; ++j) {
            const unsigned idx = tid + 256 * j, T = idx >> 2, p4 = idx & 3u;
            const unsigned pl = ((T >> 4) << 3) | (T & 7u), pair = p0 + pl;
            const bool second = ((T >> 3) & 1u) != 0;
            st_ok[j] = T < (unsigned)NLT && pair < NP && (second ? (pair >= po.p2lo && second_out) : pair < po.np1);
            const unsigned mc = st_ok[j] ? (second ? fpos2(pair) : fpos1(pair)) : 0u;   // memory column = operand line of the column pass
            st_off[j] = ((size_t)g * po.cop_lines + (size_t)z * po.W + mc) * 8u + 2u * p4;
            st_lds[j] = (T < (unsigned)NLT ? T : 0u) * 8u + 2u * (p4 ^ ((T >> 2) & 3u));
        }
        const size_t pstride = (size_t)po.cop_lines * po.cop_k16;
#pragma unroll
        for (int rnd = 0; rnd < 4; ++rnd) {
            __syncthreads();                  // the transpose areas (round 0) / the previous round's slabs have been read
            if constexpr (ENERGY) {
                // one add per (block, output): outputs that exist only (st_ok's conditions); the order of the adds is free --
                // the sums decide what is computed, never a value
                if (rnd == 0 && tid < 128) {
                    const unsigned pl = tid & 63u, pair = p0 + pl;
                    const bool second = tid >= 64;
                    const bool ok = pl < (unsigned)NPT && pair < NP && (second ? (pair >= po.p2lo && second_out) : pair < po.np1);
                    if (ok) unsafeAtomicAdd(po.col_energy + (size_t)z * po.W + (second ? fpos2(pair) : fpos1(pair)), eb[tid]);
                }
            }
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                if ((lane + 64 * c) >= (unsigned)NIT) continue;
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int i = 0; i < NI; i += 2) {
                        const unsigned ch = ((u0 + i) >> 1) ^ ((tl[c] >> 2) & 3u);
                        *reinterpret_cast<f64x2*>(slab + (a * NLT + tl[c]) * 8 + 2 * ch) = (f64x2){o[c][i][4 * rnd + a], o[c][i + 1][4 * rnd + a]};
                    }
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < NSW; ++j) {
                if (!st_ok[j]) continue;
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    const f64x2 v = *reinterpret_cast<const f64x2*>(slab + a * NLT * 8 + st_lds[j]);
                    // (non-temporal stores here: measured, no change in time or in FETCH_SIZE)
                    *reinterpret_cast<f64x2*>(po.cop + (size_t)(4 * rnd + a) * pstride + st_off[j]) = v;
                }
            }
        }
        trace_end();
        return;
    }
    // Row passes, EPI_FWD / EPI_INV_O.  While this wave stores its results the other resident block streams f64 MFMAs
    // on the same SIMD, and a VALU instruction of this wave then gets an issue slot about once per MFMA (64 cycles):
    // measured, the epilogue takes ~70 cycles per VALU instruction (tools/tile_trace.py) -- 36 us of a 125 us tile with
    // per-element bounds checks and 64-bit addresses.  So: buffer stores whose lane offsets are computed once per
    // 16-pair tile, rows advanced through the scalar offset, invalid lanes / rows dropped by the buffer's range check
    // (offset 2^31 >= num_records) instead of branches; per output element one conversion and one store.
    if constexpr (!COLS && (EPI == EPI_FWD || EPI == EPI_INV_O || EPI == EPI_INV_OT)) {
        const unsigned rows_valid = L - m0 < (unsigned)BM ? L - m0 : (unsigned)BM;
        const unsigned long long region = (unsigned long long)rows_valid * W * 4ull;
        if (region < 0x80000000ull && (EPI == EPI_FWD || (EPI == EPI_INV_O && n == W) || EPI == EPI_INV_OT)) {
            constexpr unsigned OOB = 0x80000000u;
            const bool plain = ep.first == 1.0f && ep.base == 1.0f;
            const __amdgpu_buffer_rsrc_t orr = __builtin_amdgcn_make_buffer_rsrc((void*)(po.out + (size_t)m0 * W), 0, (unsigned)region, 0x00020000);
            const unsigned swm = __builtin_amdgcn_readfirstlane(wm);
            auto st = [&](float v, unsigned voff, unsigned soff) {
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), orr, voff, soff, 0);
            };
            if constexpr (EPI == EPI_FWD) {
                unsigned vo1[NJ], vo2[NJ];
                float f1[NJ], f2[NJ];
#pragma unroll
                for (int jn = 0; jn < NJ; ++jn) {
                    const unsigned pair = p0 + wn + 16 * jn + li;
                    const unsigned i1 = fpos1(pair), i2 = fpos2(pair);
                    vo1[jn] = (pair < NP && pair < po.np1) ? (lq * W + i1) * 4u : OOB;
                    vo2[jn] = (pair < NP && pair >= po.p2lo && second_out) ? (lq * W + i2) * 4u : OOB;
                    f1[jn] = i1 == 0 ? ep.first : ep.base;
                    f2[jn] = i2 == 0 ? ep.first : ep.base;
                }
#pragma unroll
                for (int i = 0; i < NI; ++i)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const unsigned soff = (swm + 16 * i + 4 * r) * W * 4u;
#pragma unroll
                        for (int jn = 0; jn < NJ; ++jn) {
                            float v1 = (float)acc1[i][jn][r], v2 = (float)acc2[i][jn][r];
                            if (!plain) { v1 *= f1[jn]; v2 *= f2[jn]; }
                            st(v1, vo1[jn], soff);
                            st(v2, vo2[jn], soff);
                        }
                    }
            } else if constexpr (EPI == EPI_INV_OT) {
                // T[n1] = T2[n1] + a, T[n-1-n1] = T2[n1] - a as doubles (T lines: n doubles = W * 4 bytes, T2 lines half that)
                // (n = W/2: the half-length transform E; n = W/4 at level 2: its even half T2 from the folded quarter)
                const unsigned tregion = rows_valid * n * 8u;             // <= region: n <= W/2
                const __amdgpu_buffer_rsrc_t irr = __builtin_amdgcn_make_buffer_rsrc((void*)(po.tmp + (size_t)m0 * (n / 2)), 0, tregion / 2, 0x00020000);
                const __amdgpu_buffer_rsrc_t trr = __builtin_amdgcn_make_buffer_rsrc((void*)(po.tmp_out + (size_t)m0 * n), 0, tregion, 0x00020000);
                unsigned vt[NJ][2], vp[NJ][2], vm[NJ][2];
#pragma unroll
                for (int jn = 0; jn < NJ; ++jn) {
                    const unsigned pair = p0 + wn + 16 * jn + li;
#pragma unroll
                    for (int h2 = 0; h2 < 2; ++h2) {
                        const unsigned nn = h2 ? po.c2 + po.cs * p2(pair) : po.c1 + po.cs * pair;
                        const bool ok = pair < NP && nn < n / 2;
                        vt[jn][h2] = ok ? (lq * (n / 2) + tpos(nn)) * 8u : OOB;
                        vp[jn][h2] = ok ? (lq * n + opos(nn, n)) * 8u : OOB;
                        vm[jn][h2] = ok ? (lq * n + opos(n - 1 - nn, n)) * 8u : OOB;
                    }
                }
                auto std64 = [&](double v, unsigned voff, unsigned soff) {
                    const u32x2 raw = {(unsigned)__double2loint(v), (unsigned)__double2hiint(v)};
                    __builtin_amdgcn_raw_buffer_store_b64(raw, trr, voff, soff, 0);
                };
                // r6: the T2 values of line tile i + 1 are requested BEFORE the stores of line tile i (loads and stores through
                // buffer resources keep their program order: behind the stores, every line tile was a load -> wait -> store chain)
                auto load_e = [&](int i, double (&e)[4][NJ][2]) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const unsigned soff = (swm + 16 * i + 4 * r) * (n / 2) * 8u;
#pragma unroll
                        for (int jn = 0; jn < NJ; ++jn)
#pragma unroll
                            for (int h2 = 0; h2 < 2; ++h2) {
                                const u32x2 raw = __builtin_amdgcn_raw_buffer_load_b64(irr, vt[jn][h2], soff, 0);
                                e[r][jn][h2] = __hiloint2double((int)raw[1], (int)raw[0]);
                            }
                    }
                };
                double ea[4][NJ][2], eb[4][NJ][2];
                load_e(0, ea);
#pragma unroll
                for (int i = 0; i < NI; ++i) {
                    double (&e)[4][NJ][2] = (i & 1) ? eb : ea;
                    if (i + 1 < NI) load_e(i + 1, (i & 1) ? ea : eb);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const unsigned soff = (swm + 16 * i + 4 * r) * n * 8u;
#pragma unroll
                        for (int jn = 0; jn < NJ; ++jn)
#pragma unroll
                            for (int h2 = 0; h2 < 2; ++h2) {
                                const double a = h2 ? acc2[i][jn][r] : acc1[i][jn][r];
                                std64(e[r][jn][h2] + a, vp[jn][h2], soff);
                                std64(e[r][jn][h2] - a, vm[jn][h2], soff);
                            }
                    }
                }
            } else {
                // x[n1] = E[n1] + a1, x[n-1-n1] = E[n1] - a1, x[n2] = E[n2] + a2, x[n-1-n2] = E[n2] - a2; E read as doubles
                const __amdgpu_buffer_rsrc_t trr = __builtin_amdgcn_make_buffer_rsrc((void*)(po.tmp + (size_t)m0 * (n / 2)), 0, (unsigned)region, 0x00020000);
                unsigned vt[NJ][2], vp[NJ][2], vm[NJ][2];
                float fp[NJ][2];
#pragma unroll
                for (int jn = 0; jn < NJ; ++jn) {
                    const unsigned pair = p0 + wn + 16 * jn + li;
#pragma unroll
                    for (int h2 = 0; h2 < 2; ++h2) {
                        const unsigned nn = h2 ? po.c2 + po.cs * p2(pair) : po.c1 + po.cs * pair;
                        const bool ok = pair < NP && nn < n / 2;
                        vt[jn][h2] = ok ? (lq * (n / 2) + opos(nn, n / 2)) * 8u : OOB;
                        vp[jn][h2] = ok ? (lq * W + oposf(nn, n)) * 4u : OOB;
                        vm[jn][h2] = ok ? (lq * W + oposf(n - 1 - nn, n)) * 4u : OOB;
                        fp[jn][h2] = nn == 0 ? ep.first : ep.base;
                    }
                }
                auto load_e = [&](int i, double (&e)[4][NJ][2]) {                 // (one line tile ahead of the stores, as above)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const unsigned soff = (swm + 16 * i + 4 * r) * (n / 2) * 8u;
#pragma unroll
                        for (int jn = 0; jn < NJ; ++jn)
#pragma unroll
                            for (int h2 = 0; h2 < 2; ++h2) {
                                const u32x2 raw = __builtin_amdgcn_raw_buffer_load_b64(trr, vt[jn][h2], soff, 0);
                                e[r][jn][h2] = __hiloint2double((int)raw[1], (int)raw[0]);
                            }
                    }
                };
                double ea[4][NJ][2], eb[4][NJ][2];
                load_e(0, ea);
#pragma unroll
                for (int i = 0; i < NI; ++i) {
                    double (&e)[4][NJ][2] = (i & 1) ? eb : ea;
                    if (i + 1 < NI) load_e(i + 1, (i & 1) ? ea : eb);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const unsigned soff = (swm + 16 * i + 4 * r) * W * 4u;
#pragma unroll
                        for (int jn = 0; jn < NJ; ++jn)
#pragma unroll
                            for (int h2 = 0; h2 < 2; ++h2) {
                                const double a = h2 ? acc2[i][jn][r] : acc1[i][jn][r];
                                float vpl = (float)(e[r][jn][h2] + a), vmi = (float)(e[r][jn][h2] - a);
                                if (!plain) { vpl *= fp[jn][h2]; vmi *= ep.base; }
                                st(vpl, vp[jn][h2], soff);
                                st(vmi, vm[jn][h2], soff);
                            }
                    }
                }
            }
            trace_end();
            return;
        }
    }
    if constexpr (!COLS) {
#pragma unroll
        for (int jn = 0; jn < NJ; ++jn) {
            const unsigned pair = p0 + wn + 16 * jn + li;
            if (pair >= NP) continue;
#pragma unroll
            for (int i = 0; i < NI; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const unsigned row = m0 + wm + 16 * i + lq + 4 * r;
                    if (row >= L) continue;
                    emit(po.out + (size_t)row * W, po.tmp + (size_t)row * (n / 2), po.tmp_out + (size_t)row * n, 1, pair, acc1[i][jn][r], acc2[i][jn][r]);
                }
        }
    } else if constexpr (EPI == EPI_INV_E) {
      if (po.wide) {
        // The even half E of a two-level inverse column pass leaves unrounded, as doubles: T[pair] = a1 + a2,
        // T[n/2-1-pair] = a1 - a2.  Same idea as below with 8-byte elements: per round 16 result rows x CW columns of
        // one sign go through LDS (pitch CW doubles: a 16-lane ds_write_b64 group covers one 128-byte bank window)
        // and every lane stores two doubles: 512-byte row segments instead of 128-byte ones, half the stores.
        constexpr int CW = 16 * NI, DPR = CW / 2, RPI = 64 / DPR, NRI = 16 / RPI;   // double pairs per row, rows per read
        static_assert(4 * 16 * CW * 8 <= (int)sizeof(lds), "transpose area");
        __syncthreads();
        double* tw = lds + wave * (16 * CW);
        const unsigned wr0 = lq * CW + li;                                 // + (4 r) * CW + 16 i
        const unsigned dq = lane % DPR, rrow = lane / DPR;
        const unsigned line = m0 + wm + 2 * dq;                            // = frame * W + column, even
        const bool line_ok = line < L;
        const unsigned z = line_ok ? line / W : 0, col = line_ok ? line - z * W : 0;
        double* tbase = po.tmp + (size_t)z * (n / 2) * W + col;
        const double* trd = tw + rrow * CW + 2 * dq;
        auto lds_order = [&]() {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        };
#pragma unroll
        for (int jn = 0; jn < NJ; ++jn)
#pragma unroll
            for (int sign = 0; sign < 2; ++sign) {
                lds_order();
#pragma unroll
                for (int i = 0; i < NI; ++i)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        tw[wr0 + (4 * r) * CW + 16 * i] = sign ? acc1[i][jn][r] - acc2[i][jn][r] : acc1[i][jn][r] + acc2[i][jn][r];
                lds_order();
#pragma unroll
                for (int t = 0; t < NRI; ++t) {
                    const unsigned pair = p0 + wn + 16 * jn + t * RPI + rrow;
                    const f64x2 v = *reinterpret_cast<const f64x2*>(trd + t * RPI * CW);
                    if (!line_ok || pair >= NP) continue;
                    const unsigned idx = sign ? n / 2 - 1 - pair : pair;
                    *reinterpret_cast<f64x2*>(tbase + (size_t)idx * W) = v;
                }
            }
        trace_end();
        return;
      }
    } else if constexpr (EPI == EPI_INV_OT) {
      if (po.wide) {
        // Deep inverse column pass: the odd part of the half-length transform, combined with its even half T2 into T --
        // doubles out, through the same LDS transpose as EPI_INV_E (16 result rows x CW columns per round).
        constexpr int CW = 16 * NI, DPR = CW / 2, RPI = 64 / DPR, NRI = 16 / RPI;
        static_assert(4 * 16 * CW * 8 <= (int)sizeof(lds), "transpose area");
        __syncthreads();
        double* tw = lds + wave * (16 * CW);
        const unsigned wr0 = lq * CW + li;
        const unsigned dq = lane % DPR, rrow = lane / DPR;
        const unsigned line = m0 + wm + 2 * dq;
        const bool line_ok = line < L;
        const unsigned z = line_ok ? line / W : 0, col = line_ok ? line - z * W : 0;
        double* tbase = po.tmp_out + (size_t)z * n * W + col;
        const double* trd = tw + rrow * CW + 2 * dq;
        auto lds_order = [&]() {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        };
#pragma unroll
        for (int jn = 0; jn < NJ; ++jn)
#pragma unroll
            for (int h2 = 0; h2 < 2; ++h2) {
                double e[NI][4];
#pragma unroll
                for (int i = 0; i < NI; ++i) {
                    const unsigned ln = m0 + wm + 16 * i + li;
                    const unsigned lz = ln < L ? ln / W : 0, lc = ln < L ? ln - lz * W : 0;
                    const double* tp2 = po.tmp + (size_t)lz * (n / 2) * W + lc;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const unsigned pair = p0 + wn + 16 * jn + lq + 4 * r;
                        const unsigned pcl = pair < NP ? pair : 1;
                        const unsigned nn = h2 ? po.c2 + po.cs * p2(pcl) : po.c1 + po.cs * pcl;
                        e[i][r] = tp2[(size_t)(nn < n / 2 ? nn : 0) * W];
                    }
                }
#pragma unroll
                for (int sign = 0; sign < 2; ++sign) {
                    lds_order();
#pragma unroll
                    for (int i = 0; i < NI; ++i)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const double a = h2 ? acc2[i][jn][r] : acc1[i][jn][r];
                            tw[wr0 + (4 * r) * CW + 16 * i] = sign ? e[i][r] - a : e[i][r] + a;
                        }
                    lds_order();
#pragma unroll
                    for (int t = 0; t < NRI; ++t) {
                        const unsigned pair = p0 + wn + 16 * jn + t * RPI + rrow;
                        const f64x2 v = *reinterpret_cast<const f64x2*>(trd + t * RPI * CW);
                        if (!line_ok || pair >= NP) continue;
                        const unsigned nn = h2 ? po.c2 + po.cs * p2(pair) : po.c1 + po.cs * pair;
                        if (nn >= n / 2) continue;
                        const unsigned idx = sign ? n - 1 - nn : nn;
                        *reinterpret_cast<f64x2*>(tbase + (size_t)idx * W) = v;
                    }
                }
            }
        trace_end();
        return;
      }
    } else {
      if (po.wide) {
        // Column pass, wide stores.  A D tile has the image columns along the lanes, 16 at a time: stored as it is, a
        // wave writes 64-byte pieces (half cache lines, measured: the write traffic of such an epilogue costs the
        // co-resident block's main loop 4 % of a column pass).  Instead each wave transposes its results through LDS
        // -- 32 result rows x CW columns per round -- and every lane stores 16 bytes of a row: whole lines, a
        // quarter of the store instructions and of the address arithmetic.  Same values, same rounding points.
        constexpr int CW = 16 * NI;                                        // image columns of this wave's sub-tile
        constexpr int TPF = (CW % 32 == 0) ? CW + 16 : CW + 32;           // row pitch in floats: odd multiple of 16 banks
        constexpr int QPR = CW / 4, RPI = 64 / QPR, NRI = 32 / RPI;        // quads per row, rows per read, reads per round
        static_assert(4 * 32 * TPF * 4 <= (int)sizeof(lds), "transpose area");
        __syncthreads();                      // every wave has read its last fragments: the operand tiles are free
        float* tw = reinterpret_cast<float*>(lds) + wave * (32 * TPF);
        const unsigned wr0 = lq * TPF + li;                                // + (16 jn + 4 r) * TPF + 16 i
        const unsigned q = lane % QPR, rrow = lane / QPR;
        const unsigned line = m0 + wm + 4 * q;                             // = frame * W + column, a multiple of 4
        const bool line_ok = line < L;
        const unsigned z = line_ok ? line / W : 0, col = line_ok ? line - z * W : 0;
        const size_t fbase = (size_t)z * H * W + col;                      // (frame z, row 0, col) in elements
        const float* trd = tw + rrow * TPF + 4 * q;
        // LDS instructions of one wave execute in order, so a read sees the writes issued before it; the fences keep
        // the compiler from moving one across the other (it cannot see that other lanes wrote what a lane reads)
        auto lds_order = [&]() {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        };
        const bool plain = ep.first == 1.0f && ep.base == 1.0f;            // x * 1.0f is exact: skipping it changes nothing
        auto put_quad = [&](unsigned idx, f32x4 v) {                       // 4 columns of output row idx
            const float f = idx == 0 ? ep.first : ep.base;
            float y[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) y[t] = plain ? v[t] : v[t] * f;
            const size_t px = fbase + (size_t)idx * W;
            if (EPI == EPI_INV_O_RGB) pair_store_rgb_quad<double>(po, px, y);
            else *reinterpret_cast<f32x4*>(po.out + px) = (f32x4){y[0], y[1], y[2], y[3]};
        };
        if (EPI == EPI_FWD || EPI == EPI_INV) {
            // a round = up to two pair tiles (32 result rows) of one output set; NJ = 3 (48-pair tiles): a second round for the third
#pragma unroll
            for (int jb = 0; jb < NJ; jb += 2)
#pragma unroll
            for (int set = 0; set < 2; ++set) {
                const int nj2 = NJ - jb < 2 ? NJ - jb : 2;
                lds_order();
#pragma unroll
                for (int i = 0; i < NI; ++i)
#pragma unroll
                    for (int jn = jb; jn < jb + 2; ++jn) {
                        if (jn >= NJ) continue;
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const double a1 = acc1[i][jn][r], a2 = acc2[i][jn][r];
                            const float v = EPI == EPI_FWD ? (float)(set ? a2 : a1) : (float)(set ? a1 - a2 : a1 + a2);
                            tw[wr0 + (16 * (jn - jb) + 4 * r) * TPF + 16 * i] = v;
                        }
                    }
                lds_order();
#pragma unroll
                for (int t = 0; t < NRI; ++t) {
                    const unsigned srow = t * RPI + rrow;
                    const unsigned pair = p0 + wn + 16 * jb + srow;
                    const f32x4 v = *reinterpret_cast<const f32x4*>(trd + t * RPI * TPF);
                    if (!line_ok || pair >= NP || srow >= 16u * (unsigned)nj2) continue;
                    const unsigned idx = EPI == EPI_FWD ? (set ? po.c2 + po.cs * p2(pair) : po.c1 + po.cs * pair) : (set ? n - 1 - pair : pair);
                    if (EPI == EPI_FWD && (set ? (pair < po.p2lo || !second_out) : pair >= po.np1)) continue;
                    put_quad(idx, v);
                }
            }
        } else {
            // EPI_INV_O / EPI_INV_O_RGB: x[n1] = E[n1] + a1, x[n-1-n1] = E[n1] - a1, x[n2] = E[n2] + a2, x[n-1-n2] = E[n2] - a2
            // (n1 = pair, n2 = pair + n/4); a round = 16 pairs: the "+" rows in staging rows 0..15, the "-" rows in 16..31
            const double* tpl = po.tmp + (size_t)z * (n / 2) * W + (m0 + wm - z * W);      // + row * W + 16 i + li, own frame only
            // EPI_INV_O_RGB: frame of the tile's first line; `rgb_fast`: the tile's last line lies in it too
            // (the divisions run on the vector unit: without the readfirstlane the resources count as divergent and every access
            // through them is wrapped in a waterfall loop)
            const unsigned z0 = (unsigned)__builtin_amdgcn_readfirstlane((int)(m0 / W)), mlast = (m0 + BM <= L ? m0 + BM : L) - 1;
            const bool rgb_fast = EPI == EPI_INV_O_RGB && __builtin_amdgcn_readfirstlane((int)(mlast / W)) == (int)z0 &&
                                  (unsigned long long)H * W * 12ull < 0x20000000ull * 3ull;
            const size_t fpx = (size_t)z0 * H * W;
            const unsigned fbytes = H * W;
            const __amdgpu_buffer_rsrc_t rgb_i = __builtin_amdgcn_make_buffer_rsrc((void*)(po.iq_i ? po.iq_i + fpx : po.out), 0, rgb_fast ? fbytes * 4u : 0u, 0x00020000);
            const __amdgpu_buffer_rsrc_t rgb_q = __builtin_amdgcn_make_buffer_rsrc((void*)(po.iq_q ? po.iq_q + fpx : po.out), 0, rgb_fast ? fbytes * 4u : 0u, 0x00020000);
            const __amdgpu_buffer_rsrc_t rgb_o = __builtin_amdgcn_make_buffer_rsrc(
                po.rgb ? (void*)(static_cast<char*>(po.rgb) + fpx * (po.rgb_u8 ? 3u : 12u)) : (void*)po.out, 0, rgb_fast ? fbytes * (po.rgb_u8 ? 3u : 12u) : 0u, 0x00020000);
#pragma unroll
            for (int half = 0; half < 2; ++half)
#pragma unroll
                for (int jn = 0; jn < NJ; ++jn) {
                    double e[NI][4];
#pragma unroll
                    for (int i = 0; i < NI; ++i) {
                        const unsigned ln = m0 + wm + 16 * i + li;
                        const unsigned lz = ln < L ? ln / W : 0, lc = ln < L ? ln - lz * W : 0;
                        const double* tp = po.tmp + (size_t)lz * (n / 2) * W + lc;
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const unsigned pair = p0 + wn + 16 * jn + lq + 4 * r;
                            const unsigned pc = pair < NP ? pair : 0;
                            const unsigned nn = half ? po.c2 + po.cs * p2(pc) : po.c1 + po.cs * pc;
                            e[i][r] = tp[(size_t)(nn < n / 2 ? nn : 0) * W];
                        }
                    }
                    (void)tpl;
                    lds_order();
#pragma unroll
                    for (int i = 0; i < NI; ++i)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const double a = half ? acc2[i][jn][r] : acc1[i][jn][r];
                            tw[wr0 + (4 * r) * TPF + 16 * i] = (float)(e[i][r] + a);
                            tw[wr0 + (16 + 4 * r) * TPF + 16 * i] = (float)(e[i][r] - a);
                        }
                    lds_order();
                    if constexpr (EPI == EPI_INV_O_RGB) {
                        // r6: the tile's lines lie in one frame (block-uniform: W % BM == 0 for every frame size of the 4K / 8K / 1080p
                        // paths): I, Q and the pixels through buffer resources of that frame, a lane outside the tile or the class
                        // at an offset behind the range -- no branch around a load or a store, so the compiler counts its waits and
                        // the I / Q quads of RGB_NB output rows are in flight together (with the branches every quad was its own
                        // load -> wait -> store chain: `vmcnt(1)`, `vmcnt(0)` per quad in the ISA, the previous quad's stores included)
                        if (rgb_fast) {
                            // (one copy of the round per pixel format: a format branch inside it would leave the number of stores
                            // between two waits open, and the compiler would wait for the previous quad's stores as well)
                            auto rgb_round = [&](auto u8c) {
                            constexpr bool U8 = decltype(u8c)::value;
                            constexpr int NB = NRI < RGB_NB ? NRI : RGB_NB;
#pragma unroll
                            for (int tb = 0; tb < NRI; tb += NB) {
                                unsigned off[NB];
                                float fac[NB];
                                f32x4 v[NB], iv[NB], qv[NB];
#pragma unroll
                                for (int u = 0; u < NB; ++u) {
                                    const int t = tb + u;
                                    const unsigned srow = t * RPI + rrow;
                                    const unsigned pair = p0 + wn + 16 * jn + (srow & 15);
                                    v[u] = *reinterpret_cast<const f32x4*>(trd + t * RPI * TPF);
                                    const unsigned pc = pair < NP ? pair : 0;
                                    const unsigned nn = half ? po.c2 + po.cs * p2(pc) : po.c1 + po.cs * pc;
                                    const bool ok = line_ok && pair < NP && nn < n / 2;
                                    const unsigned idx = srow < 16 ? nn : n - 1 - nn;
                                    off[u] = ok ? idx * W + col : 0x20000000u;             // pixels; x 4 / x 12 / x 3 bytes stays behind every range
                                    fac[u] = idx == 0 ? ep.first : ep.base;
                                    iv[u] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rgb_i, off[u] * 4u, 0, 0));
                                    qv[u] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rgb_q, off[u] * 4u, 0, 0));
                                }
#pragma unroll
                                for (int u = 0; u < NB; ++u) {
                                    float y[4], c[12];
#pragma unroll
                                    for (int e4 = 0; e4 < 4; ++e4) y[e4] = plain ? v[u][e4] : v[u][e4] * fac[u];
                                    pair_rgb_of_quad(y, iv[u], qv[u], c);
                                    if (U8) {
                                        unsigned w3[3];
                                        pair_rgb8_words(c, w3);
                                        __builtin_amdgcn_raw_buffer_store_b96((u32x3){w3[0], w3[1], w3[2]}, rgb_o, off[u] * 3u, 0, 0);
                                    } else {
#pragma unroll
                                        for (int d = 0; d < 3; ++d)
                                            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, (f32x4){c[4 * d], c[4 * d + 1], c[4 * d + 2], c[4 * d + 3]}),
                                                                                   rgb_o, off[u] * 12u + 16u * d, 0, 0);
                                    }
                                }
                            }
                            };
                            if (po.rgb_u8) rgb_round(std::true_type{}); else rgb_round(std::false_type{});
                            continue;
                        }
                    }
#pragma unroll
                    for (int t = 0; t < NRI; ++t) {
                        const unsigned srow = t * RPI + rrow;                        // staging row: [0, 16) plus, [16, 32) minus
                        const unsigned pair = p0 + wn + 16 * jn + (srow & 15);
                        const f32x4 v = *reinterpret_cast<const f32x4*>(trd + t * RPI * TPF);
                        if (!line_ok || pair >= NP) continue;
                        const unsigned nn = half ? po.c2 + po.cs * p2(pair) : po.c1 + po.cs * pair;
                        if (nn >= n / 2) continue;
                        put_quad(srow < 16 ? nn : n - 1 - nn, v);
                    }
                }
        }
        trace_end();
        return;
      }
    }
    if constexpr (COLS) {
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const unsigned line = m0 + wm + 16 * i + li;       // = frame * W + column
            if (line >= L) continue;
            const unsigned z = line / W, col = line - z * W;
            float* lp = po.out + (size_t)z * H * W + col;
            double* tp = po.tmp + (size_t)z * (n / 2) * W + col;
            if (EPI == EPI_INV_O_RGB) {
                // Writer::result in the last pass: per pair, its 4 output rows -- the even-half values of two pairs, then
                // I and Q of a pair's four pixels, are loaded together (deeper batches spill: 198 VGPRs as it is);
                // offsets from the frame's pixel (row 0, col) address I, Q and RGB alike
                const size_t base = (size_t)z * H * W + col;
#pragma unroll
                for (int jn = 0; jn < NJ; ++jn)
#pragma unroll
                    for (int r = 0; r < 4; r += 2) {
                        double e1[2], e2[2];
                        bool ok1[2], ok2[2];
                        unsigned m1[2], m2[2];
#pragma unroll
                        for (int q = 0; q < 2; ++q) {
                            const unsigned pair = p0 + wn + 16 * jn + lq + 4 * (r + q);
                            const unsigned pc = pair < NP ? pair : 0;
                            const unsigned n1 = po.c1 + po.cs * pc, n2 = po.c2 + po.cs * p2(pc);
                            ok1[q] = pair < NP && n1 < n / 2;
                            ok2[q] = pair < NP && n2 < n / 2;
                            m1[q] = ok1[q] ? n1 : 0;
                            m2[q] = ok2[q] ? n2 : 0;
                            e1[q] = tp[(size_t)m1[q] * W];
                            e2[q] = tp[(size_t)m2[q] * W];
                        }
#pragma unroll
                        for (int q = 0; q < 2; ++q) {
                            const double a1 = acc1[i][jn][r + q], a2 = acc2[i][jn][r + q];
                            const unsigned idx1[2] = {m1[q], n - 1 - m1[q]}, idx2[2] = {m2[q], n - 1 - m2[q]};
                            const float v1[2] = {(float)(e1[q] + a1), (float)(e1[q] - a1)}, v2[2] = {(float)(e2[q] + a2), (float)(e2[q] - a2)};
                            unsigned px1[2], px2[2];
                            float y1[2], y2[2];
#pragma unroll
                            for (int o = 0; o < 2; ++o) {
                                px1[o] = idx1[o] * W; y1[o] = apply_epilogue(ep, v1[o], idx1[o]);
                                px2[o] = idx2[o] * W; y2[o] = apply_epilogue(ep, v2[o], idx2[o]);
                            }
                            pair_store_rgb_batch<double, 2>(po, base, px1, y1, ok1[q]);
                            pair_store_rgb_batch<double, 2>(po, base, px2, y2, ok2[q]);
                        }
                    }
                continue;
            }
#pragma unroll
            for (int jn = 0; jn < NJ; ++jn)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const unsigned pair = p0 + wn + 16 * jn + lq + 4 * r;
                    if (pair >= NP) continue;
                    emit(lp, tp, po.tmp_out + (size_t)z * n * W + col, W, pair, acc1[i][jn][r], acc2[i][jn][r]);
                }
        }
    }
    trace_end();
    };
    // (a tail of at most 16 pairs -- 270 = 4 x 64 + 14 at full HD, the 16-pair classes of the pruned transform -- runs
    // one 16-pair MFMA tile per wave instead of two)
    // (row passes: a tail of 33 .. 48 pairs -- 240 = 3 x 64 + 48: every launch of a 4K row pass -- runs three per wave on
    // the 4 x 1 grid: three quarters of a full tile's MFMAs)
    using J1 = std::integral_constant<int, 1>;
    using J2 = std::integral_constant<int, 2>;
    using J3 = std::integral_constant<int, 3>;
    // (tiles of 48 pairs -- po.bn32 == 2 -- always run three pair tiles on the 4 x 1 grid, whatever their valid pair count)
    const bool j3 = BM == 128 && (po.bn32 == 2 || (!COLS && NP - p0 <= 48));
    if (NP - p0 <= 16 && po.bn32 != 2) run(std::integral_constant<int, BM / 64>{}, J1{});
    else if (po.bn32 != 2 && (NP - p0 <= 32 || po.bn32)) run(std::integral_constant<int, BM / 64>{}, J2{});
    else if (j3)                       run(std::integral_constant<int, BM / 64>{}, J3{});
    else                               run(std::integral_constant<int, BM / 32>{}, J2{});
#endif
}

// Launch one of the template instances; in scope: st, ml, ep, nblk, and (below SSW_LAUNCH_PAIR_BM) `small` = 64-line tiles,
// (below SSW_LAUNCH_PAIR_SUB) inst.subname, (SSW_LAUNCH_ROWCOL) is_row.
#define SSW_LAUNCH_PAIR_BM(COLS, EPI, SAMEX, SUBV, BMV) \
        pair_gemm_f64_kernel<COLS, EPI, SAMEX, SUBV, BMV><<<(unsigned)nblk, PT, 0, st>>>(ml, ep)
#define SSW_LAUNCH_PAIR_SUB(COLS, EPI, SAMEX, SUBV) do { if (small) SSW_LAUNCH_PAIR_BM(COLS, EPI, SAMEX, SUBV, 64); else SSW_LAUNCH_PAIR_BM(COLS, EPI, SAMEX, SUBV, 128); } while (0)
#define SSW_LAUNCH_PAIR(COLS, EPI, SAMEX) do { if (inst.subname == 0) SSW_LAUNCH_PAIR_SUB(COLS, EPI, SAMEX, 0); else SSW_LAUNCH_PAIR_SUB(COLS, EPI, SAMEX, 1); } while (0)
#define SSW_LAUNCH_ROWCOL(EPI, SAMEX) do { if (is_row) SSW_LAUNCH_PAIR(false, EPI, SAMEX); else SSW_LAUNCH_PAIR(true, EPI, SAMEX); } while (0)

// the inverse instances (dct_pair_f64_inv.hip)
int launch_pair_gemm_inverse_instances(hipStream_t st, const PairMulti& ml, Epilogue ep, const PairInstance& inst, bool is_row, bool small,
                                       unsigned long long nblk);

}  // namespace ssw
