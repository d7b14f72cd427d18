// Locating scaled cut-outs whose aspect ratio was not kept exactly (ssw_locate_free_rgb8): the scale ladder of locate.hip
// answers A0 = (pw0, ph0, x0, y0) with the one height its aspect rule gives a width; this stage rescores, at full resolution, every
// size within +-a of A0 in BOTH dimensions at every position within +-4 of it, and answers the smallest SAD per pixel.
// include/ssw.h states the definition; every quantity is an integer, so nothing here depends on the order of a sum and the
// result equals the numpy restatement of tests/test_locate_free_cpu.py exactly.
//
// Kernel:
//   locate_free_kernel<C, RESIZED>   THE HOT PATH: one block = one output tile of one (suspect, size).  RESIZED: the fused
//                                    CatmullRom tile of resize_common.hpp (resize_tile_front), then horizontal pass, clamp +
//                                    round and luma as locate_rung_kernel's epilogue -- the tile's lumas land in LDS and R never
//                                    reaches HBM; the suspect's own size takes a plain luma front.  The (oyb + 8) x (oxb + 8)
//                                    patch of the original's luma plane that the clipped window can touch is staged in LDS,
//                                    byte-aligned to the window's first column while it is loaded, so every shift below is a
//                                    constant.  A thread owns words of 4 tile pixels: 3 patch words per row of the window feed
//                                    6 v_alignbyte_b32 + 9 v_sad_u8; 81 partial sums per thread, reduced in the block, one
//                                    64-bit atomic add per (block, position).
// Launch descriptors travel as kernel arguments, 32 (suspect, size) items per launch, like locate.hip's.  The final comparison
// runs on the host.
#include <algorithm>
#include <atomic>
#include <vector>

#include "locate_free_tile.hpp"
#include "ssw_host.hpp"

namespace ssw {

constexpr unsigned FREE_BATCH = 32;
constexpr unsigned FREE_SLACK_MAX = 4, FREE_MIN = 32;      // (the window and the tile: locate_free_tile.hpp)

// One (suspect, size) of a launch
struct FreeDev {
    const uint8_t* src;          // the suspect [sh][sw][C]
    uint64_t* sums;              // [FREE_POS]: position (xa + dx, ya + dy) at 9 dy + dx; zero before the launch
    ResizeTapPtrs taps;          // tables in the one buffer of the call (RESIZED)
    ResizeTile tl;
    uint32_t sw;
    uint32_t pw, ph;             // the size: R is pw x ph
    uint32_t xa, ya;             // the clipped window's first position
    uint32_t nwx, nwy;           // its positions, 1 .. 9 each
    uint32_t patch_off;          // bytes of dynamic LDS in front of the patch (a multiple of 16)
    uint32_t tile_begin;
};
struct FreeBatch { FreeDev it[FREE_BATCH]; };

__device__ inline uint32_t free_luma(uint32_t r, uint32_t g, uint32_t b) { return (77u * r + 150u * g + 29u * b + 128u) >> 8; }      // locate.hip's

// lo: the original's luma plane, rows of opitch bytes (opitch % 4 == 0), H rows, 16 bytes of slack behind the last one.
// grid: (tiles of all items of the launch); dynamic LDS: the largest item's tile + patch.
template <int C, bool RESIZED>
__global__ __launch_bounds__(256) void locate_free_kernel(FreeBatch b, unsigned n, const uint8_t* __restrict__ lo, unsigned opitch, unsigned H) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ uint32_t s_part[4][FREE_POS];
    unsigned s = 0;
    while (s + 1 < n && blockIdx.x >= b.it[s + 1].tile_begin) ++s;
    const FreeDev& d = b.it[s];
    const ResizeTile& tl = d.tl;
    const unsigned tid = threadIdx.x, tile = blockIdx.x - d.tile_begin;
    const unsigned oy0 = (tile / tl.tiles_x) * tl.oyb, ox0 = (tile % tl.tiles_x) * tl.oxb;
    const unsigned noy = d.ph - oy0 < tl.oyb ? d.ph - oy0 : tl.oyb, nox = d.pw - ox0 < tl.oxb ? d.pw - ox0 : tl.oxb;
    const unsigned nwx = d.nwx, nwy = d.nwy;

    // 1. the patch: rows ya + oy0 .. of the plane from column xa + ox0 on, shifted so that patch byte 0 IS that column.  Every
    //    byte a position of the window reads lies inside the frame (x + pw <= W, y + ph <= H); the others are never summed: the
    //    loads are clamped to the plane, not branched around
    uint32_t* s_patch = reinterpret_cast<uint32_t*>(smem + d.patch_off);
    const unsigned pp = free_patch_words(tl.oxb);
    {
        const unsigned c0 = d.xa + ox0, sh = c0 & 3, wd0 = c0 >> 2, r0 = d.ya + oy0, opw = opitch / 4, prows = noy + nwy - 1;
        const uint32_t* __restrict__ lo32 = reinterpret_cast<const uint32_t*>(lo);
        for (unsigned it = tid; it < (tl.oyb + 2 * FREE_NEAR) * pp; it += 256) {
            const unsigned r = it / pp, m = it - r * pp;
            const unsigned row = r0 + r, wd = wd0 + m;
            const bool ok = r < prows && row < H && wd < opw;
            const size_t a = (size_t)(row < H ? row : H - 1) * opw + (wd < opw ? wd : opw - 1);
            const uint32_t w0 = lo32[a], w1 = lo32[a + 1];          // a + 1: at most the first word of the slack
            s_patch[it] = ok ? __builtin_amdgcn_alignbyte(w1, w0, sh) : 0u;
        }
    }

    // 2. the tile's lumas [oyb][oxb]
    unsigned char* s_lum;
    if (RESIZED) {
        const ResizeLds l = resize_lds_carve(smem, tl, d.taps.hmax, d.taps.vmax);
        s_lum = l.in;                                      // reused after the vertical pass
        const ResizeReach rc = resize_tile_front<C>(l, d.taps, tl, tile, d.pw, d.ph, d.src, d.sw);
        const unsigned a0 = rc.a0;
        for (unsigned it = tid; it < (noy << tl.oxb_log2); it += 256) {
            const unsigned j = it >> tl.oxb_log2, x = it & ((1u << tl.oxb_log2) - 1);
            if (x >= nox) continue;
            float t[C];
            resize_horizontal_pixel<C>(l.v + j * tl.pitch + (l.lh[x] * C - a0), l.wh + x, l.ch[x], tl.oxb, t);
            s_lum[j * tl.oxb + x] = (unsigned char)free_luma(resize_to_u8(t[0]), resize_to_u8(t[1]), resize_to_u8(t[2]));
        }
    } else {
        s_lum = smem;
        for (unsigned it = tid; it < (noy << tl.oxb_log2); it += 256) {
            const unsigned j = it >> tl.oxb_log2, x = it & ((1u << tl.oxb_log2) - 1);
            if (x >= nox) continue;
            const uint8_t* __restrict__ p = d.src + ((size_t)(oy0 + j) * d.sw + ox0 + x) * C;
            s_lum[j * tl.oxb + x] = (unsigned char)free_luma(p[0], p[1], p[2]);
        }
    }
    __syncthreads();

    // 3. partial SADs: one word of 4 tile pixels against the 81 positions; bytes past nox (the tile's or the size's right edge)
    //    are masked out of both operands.  The LDS reads are unconditional (rows past the window are zeros of the patch); only
    //    the arithmetic is skipped for positions outside the clipped window (uniform)
    uint32_t acc[FREE_POS];
#pragma unroll
    for (unsigned p = 0; p < FREE_POS; ++p) acc[p] = 0;
    const unsigned kw = (nox + 3) / 4, lw = tl.oxb / 4;
    const uint32_t* s_lum32 = reinterpret_cast<const uint32_t*>(s_lum);
    for (unsigned it = tid; it < noy * kw; it += 256) {
        const unsigned j = it / kw, k = it - j * kw;
        const unsigned rem = nox - 4 * k;
        const uint32_t mask = rem >= 4 ? 0xFFFFFFFFu : (1u << (8 * rem)) - 1u;
        const uint32_t t = s_lum32[j * lw + k] & mask;
        const uint32_t* pr = s_patch + j * pp + k;
#pragma unroll
        for (unsigned dy = 0; dy < FREE_SIDE; ++dy) {
            uint32_t w[3];                                  // bytes 4 k .. 4 k + 11: dx = 0, 4, 8 are whole words, the other six are shifted
#pragma unroll
            for (unsigned q = 0; q < 3; ++q) w[q] = pr[dy * pp + q];
            if (dy < nwy) {
#pragma unroll
                for (unsigned dx = 0; dx < FREE_SIDE; ++dx) {
                    if (dx < nwx) {
                        const uint32_t win = (dx & 3) ? __builtin_amdgcn_alignbyte(w[(dx >> 2) + (dx < 8)], w[dx >> 2], dx & 3) : w[dx >> 2];
                        acc[dy * FREE_SIDE + dx] = __builtin_amdgcn_sad_u8(win & mask, t, acc[dy * FREE_SIDE + dx]);
                    }
                }
            }
        }
    }

    // 4. the block's sums (a thread's: at most 255 oyb oxb / 256, 32 bits), one atomic per position of the window
    const unsigned lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (unsigned p = 0; p < FREE_POS; ++p) {
        uint32_t v = acc[p];
#pragma unroll
        for (int o = 32; o; o >>= 1) v += __shfl_down(v, o);
        if (lane == 0) s_part[wave][p] = v;
    }
    __syncthreads();
    if (tid < FREE_POS && tid / FREE_SIDE < nwy && tid % FREE_SIDE < nwx) {
        const uint64_t total = (uint64_t)s_part[0][tid] + s_part[1][tid] + s_part[2][tid] + s_part[3][tid];
        if (total) atomicAdd(reinterpret_cast<unsigned long long*>(d.sums + tid), (unsigned long long)total);
    }
}

namespace host {

namespace {

// One (suspect, size) on the host
struct FreeItem {
    uint32_t sus, pw, ph, channels;
    bool resized;
    FreeDev dev;                 // src, sums, taps and tile_begin are filled in per launch
    TapRef vt, ht;
    uint32_t tiles;
    size_t lds;
};

// SSW_ERR_UNSUPPORTED: the resize has no LDS tile at all (the tile is chosen with the patch counted: locate_free_tile.hpp)
int make_item(LadderTaps& taps, const ssw_placement& p, uint32_t sus, uint32_t pw, uint32_t ph, uint32_t xa, uint32_t xb, uint32_t ya, uint32_t yb,
              FreeItem* out) {
    FreeItem it{};
    it.sus = sus; it.pw = pw; it.ph = ph; it.channels = p.channels;
    it.resized = pw != p.w || ph != p.h;
    FreeDev& d = it.dev;
    if (it.resized) {
        it.vt = taps.get(p.h, ph); it.ht = taps.get(p.w, pw);
        if (taps.words.size() > 0xFFFFFFFFull) return SSW_ERR_UNSUPPORTED;
    }
    if (!free_pick_tile(it.resized, it.vt.shape, it.ht.shape, pw, ph, p.channels, &d.tl, &d.patch_off, &it.lds)) return SSW_ERR_UNSUPPORTED;
    d.sw = p.w; d.pw = pw; d.ph = ph;
    d.xa = xa; d.ya = ya; d.nwx = xb - xa + 1; d.nwy = yb - ya + 1;
    it.tiles = d.tl.tiles_x * d.tl.tiles_y;
    *out = it;
    return SSW_OK;
}

// the launches of items [b0, b1) (at most FREE_BATCH): one per channel count and front that occurs
int enqueue_items(ssw_ctx* ctx, const std::vector<FreeItem>& items, size_t b0, size_t b1, const void* const* dev_suspects, uint64_t* sums,
                  const uint32_t* dev_taps, const uint8_t* lo, unsigned opitch, unsigned H) {
    static std::atomic<bool> lds_raised[64];
    SSW_TRY(resize_raise_lds_limit({reinterpret_cast<const void*>(locate_free_kernel<3, true>), reinterpret_cast<const void*>(locate_free_kernel<4, true>),
                                    reinterpret_cast<const void*>(locate_free_kernel<3, false>), reinterpret_cast<const void*>(locate_free_kernel<4, false>)},
                                   lds_raised));
    for (unsigned v = 0; v < 4; ++v) {
        const unsigned c = 3 + (v & 1);
        const bool rs = v < 2;
        FreeBatch fb{};
        unsigned m = 0, tiles = 0;
        size_t lds = 0;
        for (size_t i = b0; i < b1; ++i) {
            if (items[i].channels != c || items[i].resized != rs) continue;
            FreeDev& d = fb.it[m++];
            d = items[i].dev;
            d.src = (const uint8_t*)dev_suspects[items[i].sus];
            d.sums = sums + i * FREE_POS;
            if (rs) d.taps = resize_tap_ptrs(dev_taps, items[i].vt, items[i].ht);
            d.tile_begin = tiles;
            tiles += items[i].tiles;
            lds = std::max(lds, items[i].lds);
        }
        if (!m) continue;
        if (rs && c == 4)       locate_free_kernel<4, true><<<tiles, 256, lds, ctx->stream>>>(fb, m, lo, opitch, H);
        else if (rs)            locate_free_kernel<3, true><<<tiles, 256, lds, ctx->stream>>>(fb, m, lo, opitch, H);
        else if (c == 4)        locate_free_kernel<4, false><<<tiles, 256, lds, ctx->stream>>>(fb, m, lo, opitch, H);
        else                    locate_free_kernel<3, false><<<tiles, 256, lds, ctx->stream>>>(fb, m, lo, opitch, H);
        SSW_HIP_CHECK(hipGetLastError());
    }
    return SSW_OK;
}

// Steps 2-5 of the definition for n suspects from their starts a0 (the ladder's answers, or the start a caller of the diagnostic
// gives): the items and the luma plane, the launches, the sums back, the comparison.  Waits for the stream once.
// all_sums (ssw_locate_free_sums_rgb8; n == 1): [(2 a + 1)^2][FREE_POS], every sum of suspect 0 at its slot relative to the
// unclipped start, all ones where nothing was scored.
int free_stage(ssw_ctx* ctx, const uint8_t* dev_base, size_t w, size_t h, const void* const* dev_suspects, const std::vector<ssw_placement>& pl,
               const uint32_t* ranges, const uint32_t* slack, const ScaledAnswer* a0, ScaledAnswer* out, uint64_t* all_sums) {
    const size_t n = pl.size();
    hipStream_t st = ctx->stream;
    // sizes and windows, per suspect in the order (pw, ph): the order of the answer's ties
    LadderTaps taps;
    std::vector<FreeItem> items;
    std::vector<size_t> first(n + 1, 0);
    for (size_t i = 0; i < n; ++i) {
        const int64_t a = slack[i], wmin = ranges[2 * i], wmax = ranges[2 * i + 1];
        const ScaledAnswer& z = a0[i];
        const int64_t pw_lo = std::max<int64_t>({(int64_t)z.pw - a, wmin, (int64_t)FREE_MIN}), pw_hi = std::min<int64_t>({(int64_t)z.pw + a, wmax, (int64_t)w});
        const int64_t ph_lo = std::max<int64_t>((int64_t)z.ph - a, (int64_t)FREE_MIN), ph_hi = std::min<int64_t>((int64_t)z.ph + a, (int64_t)h);
        for (int64_t pw = pw_lo; pw <= pw_hi; ++pw)
            for (int64_t ph = ph_lo; ph <= ph_hi; ++ph) {
                const int64_t xa = std::max<int64_t>(0, (int64_t)z.x - FREE_NEAR), xb = std::min<int64_t>((int64_t)w - pw, (int64_t)z.x + FREE_NEAR);
                const int64_t ya = std::max<int64_t>(0, (int64_t)z.y - FREE_NEAR), yb = std::min<int64_t>((int64_t)h - ph, (int64_t)z.y + FREE_NEAR);
                if (xa > xb || ya > yb) continue;
                FreeItem it;
                SSW_TRY(make_item(taps, pl[i], (uint32_t)i, (uint32_t)pw, (uint32_t)ph, (uint32_t)xa, (uint32_t)xb, (uint32_t)ya, (uint32_t)yb, &it));
                items.push_back(it);
            }
        first[i + 1] = items.size();
    }
    const size_t ni = items.size();
    uint64_t* sums = nullptr;
    SSW_TRY(grow_as(ctx->locate.free_sums, std::max<size_t>(ni, 1) * FREE_POS * sizeof(uint64_t), sums));
    const unsigned opitch = (unsigned)round_up(w, 4);
    uint8_t* lo = nullptr;
    SSW_TRY(grow_as(ctx->locate.luma, (size_t)opitch * h + 16, lo));
    const uint32_t* dev_taps = nullptr;
    if (!taps.words.empty()) SSW_TRY(upload_taps(ctx, taps, &dev_taps));
    std::vector<uint64_t> hs(ni * FREE_POS);
    if (ni) {
        double bytes = (double)w * h * 4.0;
        for (const FreeItem& it : items) bytes += (double)it.dev.sw * it.channels * it.ph + (double)(it.pw + 2 * FREE_NEAR) * (it.ph + 2 * FREE_NEAR);
        StageTimer t(ctx, SSW_STAGE_LOCATE, st, bytes, SSW_STAGE_RESIZE);         // one kernel is both the resize and the search
        // the original's luma plane as locate.hip lays it out: 16 zero bytes of slack behind the last row
        SSW_HIP_CHECK(hipMemsetAsync(lo + (size_t)opitch * h, 0, 16, st));
        SSW_TRY(locate_luma_planes(ctx, dev_base, 1, w, h, lo, 0, opitch));
        SSW_HIP_CHECK(hipMemsetAsync(sums, 0, ni * FREE_POS * sizeof(uint64_t), st));
        for (size_t b0 = 0; b0 < ni; b0 += FREE_BATCH)
            SSW_TRY(enqueue_items(ctx, items, b0, std::min<size_t>(ni, b0 + FREE_BATCH), dev_suspects, sums, dev_taps, lo, opitch, (unsigned)h));
    }
    if (ni) SSW_HIP_CHECK(hipMemcpyAsync(hs.data(), sums, hs.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    untimed_work(ctx);
    SSW_HIP_CHECK(hipStreamSynchronize(st));
    // on the host: the smallest SAD / (pw ph), ties to the smaller pw, ph, y, x -- the order the candidates are visited in
    for (size_t i = 0; i < n; ++i) {
        ScaledAnswer best = a0[i];
        bool have = false;
        for (size_t q = first[i]; q < first[i + 1]; ++q) {
            const FreeDev& d = items[q].dev;
            for (uint32_t dy = 0; dy < d.nwy; ++dy)
                for (uint32_t dx = 0; dx < d.nwx; ++dx) {
                    const ScaledAnswer c{d.pw, d.ph, d.xa + dx, d.ya + dy, hs[q * FREE_POS + dy * FREE_SIDE + dx]};
                    if (!have || c.sad * ((uint64_t)best.pw * best.ph) < best.sad * ((uint64_t)c.pw * c.ph)) { best = c; have = true; }      // 255 * 2^26 * 2^26 fits 64 bits
                }
        }
        out[i] = best;
    }
    if (all_sums) {
        const int64_t a = slack[0], side = 2 * a + 1;
        std::fill(all_sums, all_sums + side * side * FREE_POS, ~0ull);
        for (size_t q = first[0]; q < first[1]; ++q) {
            const FreeDev& d = items[q].dev;
            uint64_t* slot = all_sums + (((int64_t)d.pw - a0[0].pw + a) * side + ((int64_t)d.ph - a0[0].ph + a)) * FREE_POS;
            for (uint32_t dy = 0; dy < d.nwy; ++dy)
                for (uint32_t dx = 0; dx < d.nwx; ++dx)
                    slot[(d.ya + dy + FREE_NEAR - a0[0].y) * FREE_SIDE + (d.xa + dx + FREE_NEAR - a0[0].x)] = hs[q * FREE_POS + dy * FREE_SIDE + dx];
        }
    }
    return SSW_OK;
}

}  // namespace

// pl: w, h, channels of each suspect (checked); ranges [n][2]; slack [n], each 1 .. FREE_SLACK_MAX (checked).  Waits for the stream
// three times: the ladder's two (locate_scaled_impl), and once for the sums of the stage.
int locate_free_impl(ssw_ctx* ctx, const uint8_t* dev_base, size_t w, size_t h, const void* const* dev_suspects,
                     const std::vector<ssw_placement>& pl, const uint32_t* ranges, const uint32_t* slack, ScaledAnswer* out) {
    std::vector<ScaledAnswer> a0(pl.size());
    SSW_TRY(locate_scaled_impl(ctx, dev_base, w, h, dev_suspects, pl, ranges, a0.data()));
    return free_stage(ctx, dev_base, w, h, dev_suspects, pl, ranges, slack, a0.data(), out, nullptr);
}

}  // namespace host
}  // namespace ssw

extern "C" int ssw_locate_free_rgb8(ssw_ctx* ctx, const uint8_t* dev_base_rgb, size_t w, size_t h, const void* const* dev_suspects,
                                    ssw_placement* placements, const ssw_scale_range* ranges, const uint32_t* slack, size_t n,
                                    uint64_t* host_sad) {
    using namespace ssw::host;
    if (!ctx) return SSW_ERR_BAD_ARG;
    if (n == 0) return SSW_OK;
    if (!dev_base_rgb || !dev_suspects || !placements || !ranges || !slack || !host_sad) return SSW_ERR_BAD_ARG;
    std::vector<ssw_placement> in(placements, placements + n);
    for (ssw_placement& p : in) p.x = p.y = p.pw = p.ph = 0;          // outputs: what the caller left there is not read
    if (w == 0 || h == 0 || w > 0xFFFFFFFFull || h > 0xFFFFFFFFull) return SSW_ERR_BAD_ARG;
    for (const ssw_placement& p : in)
        if ((p.channels != 3 && p.channels != 4) || p.w == 0 || p.h == 0 || (uint64_t)p.w * p.channels > 0xFFFFFFFFull) return SSW_ERR_BAD_ARG;
    for (size_t i = 0; i < n; ++i)
        if (!dev_suspects[i] || slack[i] < 1 || slack[i] > ssw::FREE_SLACK_MAX) return SSW_ERR_BAD_ARG;
    CtxGuard g(ctx);
    std::vector<ScaledAnswer> ans(n);
    std::vector<uint32_t> r(2 * n);
    for (size_t i = 0; i < n; ++i) { r[2 * i] = ranges[i].wmin; r[2 * i + 1] = ranges[i].wmax; }
    SSW_TRY(locate_free_impl(ctx, dev_base_rgb, w, h, dev_suspects, in, r.data(), slack, ans.data()));
    for (size_t i = 0; i < n; ++i) {
        placements[i].pw = ans[i].pw; placements[i].ph = ans[i].ph;
        placements[i].x = ans[i].x; placements[i].y = ans[i].y;
        host_sad[i] = ans[i].sad;
    }
    return SSW_OK;
}

extern "C" int ssw_locate_free_sums_rgb8(ssw_ctx* ctx, const uint8_t* dev_base_rgb, size_t w, size_t h, const void* dev_suspect, size_t sw, size_t sh,
                                         size_t channels, const uint32_t start[4], uint32_t wmin, uint32_t wmax, uint32_t slack, uint64_t* host_sums,
                                         ssw_placement* answer, uint64_t* host_sad) {
    using namespace ssw::host;
    if (!ctx || !dev_base_rgb || !dev_suspect || !start || !host_sums || !answer || !host_sad) return SSW_ERR_BAD_ARG;
    if (w == 0 || h == 0 || w > 0xFFFFFFFFull || h > 0xFFFFFFFFull) return SSW_ERR_BAD_ARG;
    if ((channels != 3 && channels != 4) || sw == 0 || sh == 0 || sh > 0xFFFFFFFFull || (uint64_t)sw * channels > 0xFFFFFFFFull) return SSW_ERR_BAD_ARG;
    if (slack < 1 || slack > ssw::FREE_SLACK_MAX || wmin > wmax) return SSW_ERR_BAD_ARG;
    if (start[0] == 0 || start[1] == 0 || start[0] > w || start[1] > h || start[2] > w - start[0] || start[3] > h - start[1]) return SSW_ERR_BAD_ARG;
    CtxGuard g(ctx);
    ssw_placement p{};
    p.w = (uint32_t)sw; p.h = (uint32_t)sh; p.channels = (uint32_t)channels;
    const std::vector<ssw_placement> pl(1, p);
    const uint32_t range[2] = {wmin, wmax};
    const ScaledAnswer a0{start[0], start[1], start[2], start[3], 0};
    ScaledAnswer ans{};
    SSW_TRY(free_stage(ctx, dev_base_rgb, w, h, &dev_suspect, pl, range, &slack, &a0, &ans, host_sums));
    p.pw = ans.pw; p.ph = ans.ph; p.x = ans.x; p.y = ans.y;
    *answer = p;
    *host_sad = ans.sad;
    return SSW_OK;
}
