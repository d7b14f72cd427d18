// Restoration of attacked copies before tracing (ssw_restore_rgb8): a suspect that was scaled, or cut out of the original,
// is resized back into the rectangle of the original's frame it covers and composited over the original -- the recipes of
// the reference's two attack tests,
//   imageops::resize(.., CatmullRom)                     tests/attack_resize.rs:31-36
//   "complement the attacked image with the original"    tests/attack_crop.rs:56-70   (Pixel::blend, :63)
// Like the resize, Rgba<u8>::blend is arithmetic of the third-party crate `image 0.24.3`, restated from its published
// behaviour (parity unpinned: the reference's test only exercises alpha 0 and 255; include/ssw.h states the formula).
// This file is compiled with -ffp-contract=off like the colour kernels: no product of the blend is contracted into an FMA.
//
// Two kernels, both bound by HBM bytes:
//   restore_place_kernel    no resize: whole frames [n][H][W][3] in one streaming launch -- O outside the rectangle, S (3 or
//                           4 B/px) blended inside.  For a resized suspect it writes only the outside of the rectangle.
//   restore_resize_kernel   the fused CatmullRom tile of resize_common.hpp (resize_tile_front: tile -> LDS, vertical pass into
//                           an f32 strip that never leaves the CU) with 3 or 4 input channels; its own part is the horizontal
//                           pass with the blend against O as its epilogue and an output that lands in a rectangle of a larger
//                           frame.  LDS layout, reach, loader, accumulation and rounding come from that header, which
//                           attack.hip and locate.hip use too.
// Neither kernel assumes any alignment: 32-bit accesses are taken where an address IS 4-byte aligned, bytes elsewhere.
#include <algorithm>
#include <atomic>
#include <map>
#include <tuple>
#include <vector>

#include "resize_common.hpp"
#include "ssw_host.hpp"

namespace ssw {

// one suspect of a launch; the descriptors travel as kernel arguments (no buffer to keep alive, no synchronisation)
struct RestoreDev {
    const uint8_t* src;          // the suspect [sh][sw][c]
    uint8_t* out;                // its restored frame [H][W][3]
    uint32_t sw, c;              // (place kernel) the suspect's row length in pixels, channels
    uint32_t x, y, pw, ph;       // rectangle of the frame
    uint32_t outside_only;       // (place kernel) write the frame outside the rectangle only: a resize launch fills the inside
};
constexpr unsigned RESTORE_BATCH = 32;
struct RestoreBatch { RestoreDev it[RESTORE_BATCH]; };

// rgb(blend(opaque bg, fg with alpha a)) of one channel, 0 < a < 255: Rgba<u8>::blend in f32, every operation rounded on its own
__device__ inline uint32_t blend_channel(uint32_t bg8, uint32_t fg8, float fa, float af) {
    const float ba = 1.0f;
    const float bg = (float)bg8 / 255.0f, fg = (float)fg8 / 255.0f;
    const float out = ((fg * fa) + (bg * ba) * (1.0f - fa)) / af;
    return (uint32_t)(255.0f * out) & 0xFFu;                      // truncated toward zero (NumCast); never reaches 256
}
// one pixel: o = the original's bytes, r = the suspect's (r[3] = alpha); result in o
__device__ inline void blend_pixel(uint32_t (&o)[3], const uint32_t (&r)[4]) {
    if (r[3] == 0) return;
    if (r[3] == 255) { o[0] = r[0]; o[1] = r[1]; o[2] = r[2]; return; }
    const float fa = (float)r[3] / 255.0f, ba = 1.0f;
    const float af = ba + fa - ba * fa;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = blend_channel(o[c], r[c], fa, af);
}

__device__ inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

// One thread = 4 consecutive pixels of one frame row (12 output bytes).  grid: (quads of a row / 256, H, suspects).
__global__ __launch_bounds__(256) void restore_place_kernel(const uint8_t* __restrict__ base, unsigned W, unsigned H, RestoreBatch b) {
    const RestoreDev& d = b.it[blockIdx.z];
    const unsigned x0 = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (x0 >= W) return;
    const unsigned npx = W - x0 < 4 ? W - x0 : 4;
    for (unsigned row = blockIdx.y; row < H; row += gridDim.y) {
        const bool in_row = row >= d.y && row < d.y + d.ph;
        bool in[4];
        unsigned n_in = 0;
#pragma unroll
        for (int p = 0; p < 4; ++p) { in[p] = in_row && (unsigned)p < npx && x0 + p >= d.x && x0 + p < d.x + d.pw; n_in += in[p]; }
        if (d.outside_only && n_in == npx) continue;
        const size_t off = ((size_t)row * W + x0) * 3;
        const uint8_t* __restrict__ op = base + off;
        uint8_t* __restrict__ dst = d.out + off;
        const bool full = npx == 4;
        uint32_t px[4][3];
        // the original: wanted wherever the suspect does not simply replace it
        if (!(n_in == npx && d.c == 3 && !d.outside_only)) {
            if (full && aligned4(op)) {
                const uint32_t* o32 = reinterpret_cast<const uint32_t*>(op);
                const uint32_t w0 = o32[0], w1 = o32[1], w2 = o32[2];
                px[0][0] = w0 & 0xFF; px[0][1] = (w0 >> 8) & 0xFF; px[0][2] = (w0 >> 16) & 0xFF;
                px[1][0] = w0 >> 24;  px[1][1] = w1 & 0xFF;        px[1][2] = (w1 >> 8) & 0xFF;
                px[2][0] = (w1 >> 16) & 0xFF; px[2][1] = w1 >> 24; px[2][2] = w2 & 0xFF;
                px[3][0] = (w2 >> 8) & 0xFF;  px[3][1] = (w2 >> 16) & 0xFF; px[3][2] = w2 >> 24;
            } else {
#pragma unroll
                for (int p = 0; p < 4; ++p)
                    if ((unsigned)p < npx) { px[p][0] = op[3 * p]; px[p][1] = op[3 * p + 1]; px[p][2] = op[3 * p + 2]; }
            }
        }
        if (!d.outside_only && n_in) {
            const uint8_t* __restrict__ sp = d.src + ((size_t)(row - d.y) * d.sw) * d.c;     // the suspect's row; pixel x0 + p is at (x0 + p - d.x) * c
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                if (!in[p]) continue;
                const uint8_t* s = sp + (size_t)(x0 + p - d.x) * d.c;
                if (d.c == 4) {
                    uint32_t r[4];
                    if (aligned4(s)) { const uint32_t v = *reinterpret_cast<const uint32_t*>(s); r[0] = v & 0xFF; r[1] = (v >> 8) & 0xFF; r[2] = (v >> 16) & 0xFF; r[3] = v >> 24; }
                    else { r[0] = s[0]; r[1] = s[1]; r[2] = s[2]; r[3] = s[3]; }
                    blend_pixel(px[p], r);
                } else {
                    px[p][0] = s[0]; px[p][1] = s[1]; px[p][2] = s[2];
                }
            }
        }
        if (full && !(d.outside_only && n_in) && aligned4(dst)) {
            uint32_t* o32 = reinterpret_cast<uint32_t*>(dst);
            o32[0] = px[0][0] | (px[0][1] << 8) | (px[0][2] << 16) | (px[1][0] << 24);
            o32[1] = px[1][1] | (px[1][2] << 8) | (px[2][0] << 16) | (px[2][1] << 24);
            o32[2] = px[2][2] | (px[3][0] << 8) | (px[3][1] << 16) | (px[3][2] << 24);
        } else {
#pragma unroll
            for (int p = 0; p < 4; ++p)
                if ((unsigned)p < npx && !(d.outside_only && in[p])) {
                    dst[3 * p] = (uint8_t)px[p][0]; dst[3 * p + 1] = (uint8_t)px[p][1]; dst[3 * p + 2] = (uint8_t)px[p][2];
                }
        }
    }
}

// One block = one tile of OYB x OXB pixels of the rectangle of one suspect; every suspect of a launch has the same size,
// channel count and rectangle size (one pair of tap tables).  grid: (tiles, suspects).
template <int C>
__global__ __launch_bounds__(256) void restore_resize_kernel(const uint8_t* __restrict__ base, unsigned W, RestoreBatch b, unsigned sw,
                                                             unsigned pw, unsigned ph, ResizeTapPtrs taps, ResizeTile tl) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const ResizeLds l = resize_lds_carve(smem, tl, taps.hmax, taps.vmax);
    unsigned char* s_out = l.in;                       // reused after the vertical pass: [oyb][oxb * 3]

    const RestoreDev& d = b.it[blockIdx.y];
    const unsigned tid = threadIdx.x, lane = tid & 63;
    const unsigned wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // 1. tap tables and input tile -> LDS, 2. vertical pass
    const ResizeReach rc = resize_tile_front<C>(l, taps, tl, blockIdx.x, pw, ph, d.src, sw);
    const unsigned oy0 = rc.oy0, ox0 = rc.ox0, noy = rc.noy, nox = rc.nox, a0 = rc.a0;
    // 3. horizontal pass, clamp + round of every channel, then the blend against the original; staged in LDS
    const unsigned out_pitch = tl.oxb * 3;
    for (unsigned it = tid; it < (noy << tl.oxb_log2); it += 256) {
        const unsigned j = it >> tl.oxb_log2, x = it & ((1u << tl.oxb_log2) - 1);
        if (x >= nox) continue;
        float t[C];
        resize_horizontal_pixel<C>(l.v + j * tl.pitch + (l.lh[x] * C - a0), l.wh + x, l.ch[x], tl.oxb, t);
        uint32_t r[4] = {resize_to_u8(t[0]), resize_to_u8(t[1]), resize_to_u8(t[2]), 255u};
        uint32_t o[3] = {r[0], r[1], r[2]};
        if (C == 4) {
            r[3] = resize_to_u8(t[C - 1]);
            if (r[3] != 255u) {
                const uint8_t* op = base + ((size_t)(d.y + oy0 + j) * W + (d.x + ox0 + x)) * 3;
                o[0] = op[0]; o[1] = op[1]; o[2] = op[2];
                blend_pixel(o, r);
            }
        }
        unsigned char* q = s_out + j * out_pitch + x * 3;
        q[0] = (unsigned char)o[0]; q[1] = (unsigned char)o[1]; q[2] = (unsigned char)o[2];
    }
    __syncthreads();
    // 4. tile rows -> the rectangle of the frame: 32-bit stores on rows that start 4-byte aligned, bytes on the others
    const unsigned obytes = nox * 3;
    for (unsigned j = wave; j < noy; j += 4) {
        uint8_t* drow = d.out + ((size_t)(d.y + oy0 + j) * W + (d.x + ox0)) * 3;
        const unsigned char* srow = s_out + j * out_pitch;
        if (aligned4(drow)) {
            for (unsigned wd = lane; wd < obytes / 4; wd += 64) *reinterpret_cast<uint32_t*>(drow + 4 * wd) = *reinterpret_cast<const uint32_t*>(srow + 4 * wd);
            for (unsigned e = (obytes & ~3u) + lane; e < obytes; e += 64) drow[e] = srow[e];
        } else {
            for (unsigned e = lane; e < obytes; e += 64) drow[e] = srow[e];
        }
    }
}

namespace host {

namespace {

bool whole_frame(const ssw_placement& p, size_t w, size_t h) { return p.x == 0 && p.y == 0 && p.pw == w && p.ph == h; }
bool resized(const ssw_placement& p) { return p.pw != p.w || p.ph != p.h; }

// the tile of one class of resized suspects; false: no tile fits (a suspect far larger than its rectangle)
bool restore_tile(const DeviceTaps& vt, const DeviceTaps& ht, const ssw_placement& p, ResizeTile* tl, size_t* lds) {
    if (!pick_resize_tile(vt, ht, std::max<size_t>(p.pw, 2), p.ph, p.channels, tl, lds)) return false;
    tl->tiles_x = (p.pw + tl->oxb - 1) / tl->oxb;
    tl->tiles_y = (p.ph + tl->oyb - 1) / tl->oyb;
    return true;
}

}  // namespace

bool restore_untouched(const ssw_placement& p, size_t w, size_t h) { return p.channels == 3 && p.w == w && p.h == h && whole_frame(p, w, h); }
bool restore_reads_base(const ssw_placement& p, size_t w, size_t h) { return p.channels == 4 || !whole_frame(p, w, h); }

int restore_normalise(const ssw_placement* pl, size_t n, size_t w, size_t h, std::vector<ssw_placement>* out) {
    if (n && !pl) return SSW_ERR_BAD_ARG;
    if (w == 0 || h == 0 || w > 0xFFFFFFFFull || h > 0xFFFFFFFFull) return SSW_ERR_BAD_ARG;
    out->assign(pl, pl + n);
    for (ssw_placement& p : *out) {
        if (p.channels != 3 && p.channels != 4) return SSW_ERR_BAD_ARG;
        if (p.w == 0 || p.h == 0) return SSW_ERR_BAD_ARG;
        if ((p.pw == 0) != (p.ph == 0)) return SSW_ERR_BAD_ARG;          // a rectangle of zero width or height
        if (p.pw == 0) { p.pw = p.w; p.ph = p.h; }
        if ((uint64_t)p.x + p.pw > w || (uint64_t)p.y + p.ph > h) return SSW_ERR_BAD_ARG;
        if ((uint64_t)p.w * p.channels > 0xFFFFFFFFull) return SSW_ERR_BAD_ARG;
    }
    return SSW_OK;
}

int restore_prepare(ssw_ctx* ctx, const std::vector<ssw_placement>& pl) {
    for (const ssw_placement& p : pl) {
        if (!resized(p)) continue;
        DeviceTaps vt, ht;
        SSW_TRY(get_taps(ctx, p.h, p.ph, &vt));
        SSW_TRY(get_taps(ctx, p.w, p.pw, &ht));
        ResizeTile tl;
        size_t lds = 0;
        if (!restore_tile(vt, ht, p, &tl, &lds)) return SSW_ERR_UNSUPPORTED;
    }
    return SSW_OK;
}

int restore_enqueue(ssw_ctx* ctx, const uint8_t* dev_base, size_t w, size_t h, const RestoreJob* jobs, size_t n) {
    if (!n) return SSW_OK;
    double bytes = 0.0;
    std::vector<RestoreDev> place;
    std::map<std::tuple<uint32_t, uint32_t, uint32_t, uint32_t, uint32_t>, std::vector<RestoreDev>> classes;
    for (size_t i = 0; i < n; ++i) {
        const ssw_placement& p = jobs[i].p;
        const RestoreDev d{jobs[i].src, jobs[i].out, p.w, p.channels, p.x, p.y, p.pw, p.ph, resized(p) ? 1u : 0u};
        const double rect = (double)p.pw * p.ph, frame = (double)w * h;
        if (resized(p)) {
            classes[std::make_tuple(p.w, p.h, p.pw, p.ph, p.channels)].push_back(d);
            if (!whole_frame(p, w, h)) place.push_back(d);
            bytes += (double)p.w * p.h * p.channels + 3.0 * rect + 6.0 * (frame - rect) + (p.channels == 4 ? 3.0 * rect : 0.0);
        } else {
            place.push_back(d);
            bytes += 3.0 * frame + (double)p.channels * rect + 3.0 * (frame - rect) + (p.channels == 4 ? 3.0 * rect : 0.0);
        }
    }
    StageTimer t(ctx, SSW_STAGE_RESIZE, ctx->stream, bytes);
    for (size_t i0 = 0; i0 < place.size(); i0 += RESTORE_BATCH) {
        const size_t m = std::min<size_t>(RESTORE_BATCH, place.size() - i0);
        RestoreBatch b{};
        std::copy(place.begin() + i0, place.begin() + i0 + m, b.it);
        const size_t quads = (w + 3) / 4;
        const unsigned rows = (unsigned)std::min<size_t>(h, 65535);       // grid.y limit: taller frames stride over their rows
        restore_place_kernel<<<dim3((unsigned)((quads + 255) / 256), rows, (unsigned)m), 256, 0, ctx->stream>>>(dev_base, (unsigned)w, (unsigned)h, b);
        SSW_HIP_CHECK(hipGetLastError());
    }
    static std::atomic<bool> lds_raised[64];
    if (!classes.empty())
        SSW_TRY(resize_raise_lds_limit({reinterpret_cast<const void*>(restore_resize_kernel<3>), reinterpret_cast<const void*>(restore_resize_kernel<4>)}, lds_raised));
    for (auto& kv : classes) {
        const std::vector<RestoreDev>& v = kv.second;
        const ssw_placement p{std::get<0>(kv.first), std::get<1>(kv.first), std::get<4>(kv.first), 0, 0, std::get<2>(kv.first), std::get<3>(kv.first)};
        DeviceTaps vt, ht;
        SSW_TRY(get_taps(ctx, p.h, p.ph, &vt));
        SSW_TRY(get_taps(ctx, p.w, p.pw, &ht));
        ResizeTile tl;
        size_t lds = 0;
        if (!restore_tile(vt, ht, p, &tl, &lds)) return SSW_ERR_UNSUPPORTED;
        const ResizeTapPtrs taps = resize_tap_ptrs(vt, ht);
        for (size_t i0 = 0; i0 < v.size(); i0 += RESTORE_BATCH) {
            const size_t m = std::min<size_t>(RESTORE_BATCH, v.size() - i0);
            RestoreBatch b{};
            std::copy(v.begin() + i0, v.begin() + i0 + m, b.it);
            const dim3 grid(tl.tiles_x * tl.tiles_y, (unsigned)m);
            if (p.channels == 4) restore_resize_kernel<4><<<grid, 256, lds, ctx->stream>>>(dev_base, (unsigned)w, b, p.w, p.pw, p.ph, taps, tl);
            else                 restore_resize_kernel<3><<<grid, 256, lds, ctx->stream>>>(dev_base, (unsigned)w, b, p.w, p.pw, p.ph, taps, tl);
            SSW_HIP_CHECK(hipGetLastError());
        }
    }
    return SSW_OK;
}

}  // namespace host
}  // namespace ssw

extern "C" int ssw_restore_rgb8(ssw_ctx* ctx, const uint8_t* dev_base_rgb, size_t w, size_t h, const void* const* dev_suspects,
                                const ssw_placement* placements, size_t n, uint8_t* dev_out) {
    using namespace ssw::host;
    if (!ctx) return SSW_ERR_BAD_ARG;
    if (n == 0) return SSW_OK;
    if (!dev_base_rgb || !dev_suspects || !placements || !dev_out) return SSW_ERR_BAD_ARG;
    std::vector<ssw_placement> pl;
    SSW_TRY(restore_normalise(placements, n, w, h, &pl));
    for (size_t i = 0; i < n; ++i) if (!dev_suspects[i]) return SSW_ERR_BAD_ARG;
    CtxGuard g(ctx);
    SSW_TRY(restore_prepare(ctx, pl));
    const size_t fb = w * h * 3;
    std::vector<RestoreJob> jobs;
    for (size_t i = 0; i < n; ++i) {
        if (restore_untouched(pl[i], w, h)) {       // the crate copies when nothing changes: no restore launch
            SSW_HIP_CHECK(hipMemcpyAsync(dev_out + i * fb, dev_suspects[i], fb, hipMemcpyDeviceToDevice, ctx->stream));
            untimed_work(ctx);
        } else {
            jobs.push_back(RestoreJob{(const uint8_t*)dev_suspects[i], dev_out + i * fb, pl[i]});
        }
    }
    return restore_enqueue(ctx, dev_base_rgb, w, h, jobs.data(), jobs.size());
}
