// The rotation attack and its undoing (ssw_affine_rgb8, ssw_rotate_attack_rgb8, ssw_unrotate_rgb8): a frame as
// PIL.Image.transform(AFFINE) -- and with it PIL.Image.rotate -- makes it, and a rotated copy turned back by the known angle and
// completed with the original where the turn lost pixels.  include/ssw.h states the definition; it is Pillow's Geometry.c in
// IEEE doubles, every operation rounded on its own (this file is built without contraction, and says so again below), so the
// frames equal the numpy restatement of tests/test_rotate_cpu.py -- and with it Pillow -- exactly.  The reference has no
// counterpart.
//
// One kernel family, affine_kernel<FILTER, LDS, UNDO> (grid z: the frames of a launch, AFFINE_BATCH at most):
//   a block takes a tile of AFFINE_TILE_W x AFFINE_TILE_H output pixels, a thread one pixel (three byte stores; the packed store
//   of DESIGN 4.16 was not tried again).  LDS: the block works out the box of source pixels its tile can read from the sample
//   points of the tile's four corners (affine_tile_box, the same code the host's plan bounds) and stages it, rows of `pitch`
//   bytes loaded as dwords at whatever alignment the frame has; every tap is then an LDS byte.  !LDS: the taps come from global
//   memory -- the form for matrices whose box does not fit (a strong shrink).  The inside test is made on the doubles, before
//   any conversion to an integer; a tap index is clamped to the frame, and in the LDS form to the box as well.
//   UNDO: the transform by `m` (BICUBIC), then the mask of include/ssw.h -- the footprint needs no clamping and `fwd` puts its
//   four corners inside --, and where the mask fails the original's byte: one launch, no frame in between.
// affine_cutout_kernel: the undoing of a cut-out of a turned copy (ssw_restore_turned_rgb8) -- a source of another size than the
//   output, the mask the footprint alone; a kernel of its own, so that the family above compiles to what it compiled to before.
#include <algorithm>
#include <cmath>
#include <vector>

#include "affine_tables.hpp"
#include "ssw_host.hpp"
#include "turned_tables.hpp"

#pragma clang fp contract(off)

namespace ssw {

constexpr unsigned AFFINE_BATCH = 32;                       // frames per launch, and jobs per workspace group
constexpr size_t AFFINE_GROUP_BYTES = (size_t)64 << 20;     // attacked frames kept at a time (one job's, if it is larger)
constexpr size_t AFFINE_SIDE_MAX = 65535;
constexpr unsigned AFFINE_THREADS = AFFINE_TILE_W * AFFINE_TILE_H;

struct AffineFrames { uint32_t src[AFFINE_BATCH]; };        // the frame of the input that result z of the launch is made of
struct AffineArgs {
    double m[6];
    double fwd[6];              // UNDO: the matrix that made the suspect
    uint32_t w, h, ow, oh;
    uint32_t box_w, box_h, pitch;
    uint8_t fill[4];
};

// The source as a thread sees it: bytes of the frame, or of the staged box
template <bool LDS> struct AffineSource;
template <> struct AffineSource<false> {
    const uint8_t* __restrict__ p; uint32_t w;
    __device__ double at(int i, int j, int c) const { return (double)p[((size_t)j * w + (size_t)i) * 3 + c]; }
};
template <> struct AffineSource<true> {
    const uint8_t* p; int x0, y0, bw, bh; uint32_t pitch;
    __device__ double at(int i, int j, int c) const {
        const int li = min(max(i - x0, 0), bw - 1), lj = min(max(j - y0, 0), bh - 1);
        return (double)p[(unsigned)lj * pitch + (unsigned)li * 3 + c];
    }
};

__device__ inline double af_lerp(double a, double b, double d) { return a + (b - a) * d; }
__device__ inline double af_cubic(double a, double b, double c, double d, double t) {
    const double p1 = b, p2 = -a + c, p3 = 2.0 * (a - b) + c - d, p4 = -a + b - c + d;
    return p1 + t * (p2 + t * (p3 + t * p4));
}

// one channel of one pixel: (x, y) the base position, dx, dy the fractions
template <int FILTER, class Src>
__device__ inline uint8_t af_sample(const Src& s, int x, int y, double dx, double dy, int w, int h, int c) {
    const auto XC = [&](int i) { return min(max(i, 0), w - 1); };
    const auto YC = [&](int j) { return min(max(j, 0), h - 1); };
    if (FILTER == AFFINE_BILINEAR) {
        const int xa = XC(x), xb = XC(x + 1);
        const double v1 = af_lerp(s.at(xa, YC(y), c), s.at(xb, YC(y), c), dx);
        double v2 = v1;
        if (y + 1 >= 0 && y + 1 < h) v2 = af_lerp(s.at(xa, y + 1, c), s.at(xb, y + 1, c), dx);
        return (uint8_t)(int)af_lerp(v1, v2, dy);
    }
    const int x0 = XC(x - 1), x1 = XC(x), x2 = XC(x + 1), x3 = XC(x + 2);
    const auto row = [&](int j) { const int jj = YC(j); return af_cubic(s.at(x0, jj, c), s.at(x1, jj, c), s.at(x2, jj, c), s.at(x3, jj, c), dx); };
    const double v1 = row(y - 1);
    const double v2 = (y >= 0 && y < h) ? row(y) : v1;
    const double v3 = (y + 1 >= 0 && y + 1 < h) ? row(y + 1) : v2;
    const double v4 = (y + 2 >= 0 && y + 2 < h) ? row(y + 2) : v3;
    const double v = af_cubic(v1, v2, v3, v4, dy);
    return v <= 0.0 ? (uint8_t)0 : v >= 255.0 ? (uint8_t)255 : (uint8_t)(int)v;
}

// Whether the undoing keeps pixel (X, Y): the way back's (a.m) sample point is inside, the footprint at its base position needs
// no clamping and the way there (a.fwd) puts the footprint's four corners inside.  For the count; affine_kernel<.., UNDO> has the
// same lines in its body: called from there, as a function of any shape, they cost the kernel 14.2 ms where 9.0 ms is measured
// with them in place (64 4K frames; the optimiser then arranges the sixteen taps differently).
__device__ inline bool af_undo_keeps(const AffineArgs& a, uint32_t X, uint32_t Y) {
    double xin, yin;
    affine_point(a.m, X, Y, xin, yin);
    if (!affine_inside(xin, yin, a.w, a.h)) return false;
    const int x = (int)floor(xin - 0.5), y = (int)floor(yin - 0.5);
    bool keep = x - 1 >= 0 && x + 2 <= (int)a.w - 1 && y - 1 >= 0 && y + 2 <= (int)a.h - 1;
    for (int k = 0; k < 4 && keep; ++k) {
        double fxin, fyin;
        affine_point(a.fwd, (uint32_t)((k & 1) ? x + 2 : x - 1), (uint32_t)((k & 2) ? y + 2 : y - 1), fxin, fyin);
        keep = affine_inside(fxin, fyin, a.w, a.h);
    }
    return keep;
}

// grid: (tiles across, tiles down, frames of the launch); block: AFFINE_THREADS.  in: frames [h][w][3] `in_fb` bytes apart, frame
// fr.src[z] for result z; out: [z][oh][ow][3].  base (UNDO; ow == w, oh == h): the original [h][w][3].  LDS form: dynamic LDS
// a.pitch * a.box_h bytes.
template <int FILTER, bool LDS, bool UNDO>
__global__ __launch_bounds__(AFFINE_THREADS) void affine_kernel(AffineFrames fr, AffineArgs a, const uint8_t* __restrict__ in, size_t in_fb,
                                                                const uint8_t* __restrict__ base, uint8_t* __restrict__ out, size_t out_fb) {
    extern __shared__ __attribute__((aligned(16))) uint8_t af_smem[];
    const unsigned t = threadIdx.x;
    const uint32_t X0 = blockIdx.x * AFFINE_TILE_W, Y0 = blockIdx.y * AFFINE_TILE_H;
    const uint32_t X = X0 + t % AFFINE_TILE_W, Y = Y0 + t / AFFINE_TILE_W;
    const uint8_t* __restrict__ src = in + (size_t)fr.src[blockIdx.z] * in_fb;
    AffineSource<LDS> s;
    if constexpr (LDS) {
        AffineBox b = affine_tile_box(a.m, X0, Y0, min(X0 + AFFINE_TILE_W, a.ow) - 1, min(Y0 + AFFINE_TILE_H, a.oh) - 1, a.w, a.h);
        b.bw = min(b.bw, (int)a.box_w);                     // (the plan's bound holds; the staged box never outgrows the LDS)
        b.bh = min(b.bh, (int)a.box_h);
        const size_t row_bytes = (size_t)a.w * 3;
        const uint8_t* __restrict__ sp = src + (size_t)b.y0 * row_bytes + (size_t)b.x0 * 3;
        const unsigned span = 3 * (unsigned)b.bw, dwords = span / 4, tail = span - 4 * dwords, rows = (unsigned)b.bh;
        for (unsigned i = t; i < rows * dwords; i += AFFINE_THREADS) {
            const unsigned r = i / dwords, d = i - r * dwords;
            uint32_t v;
            __builtin_memcpy(&v, sp + r * row_bytes + 4 * d, 4);
            *reinterpret_cast<uint32_t*>(af_smem + r * a.pitch + 4 * d) = v;
        }
        for (unsigned i = t; i < rows * tail; i += AFFINE_THREADS) {
            const unsigned r = i / tail, j = 4 * dwords + (i - r * tail);
            af_smem[r * a.pitch + j] = sp[r * row_bytes + j];
        }
        __syncthreads();
        s.p = af_smem; s.x0 = b.x0; s.y0 = b.y0; s.bw = b.bw; s.bh = b.bh; s.pitch = a.pitch;
    } else {
        s.p = src; s.w = a.w;
    }
    if (X >= a.ow || Y >= a.oh) return;
    uint8_t* __restrict__ dst = out + (size_t)blockIdx.z * out_fb + ((size_t)Y * a.ow + X) * 3;
    const uint8_t* __restrict__ other = UNDO ? base + ((size_t)Y * a.w + X) * 3 : a.fill;
    double xin, yin;
    affine_point(a.m, X, Y, xin, yin);
    bool keep = affine_inside(xin, yin, a.w, a.h);          // on the doubles, before any conversion
    int x = 0, y = 0;
    double dx = 0.0, dy = 0.0;
    if (keep) {
        xin -= 0.5; yin -= 0.5;
        const double fx = floor(xin), fy = floor(yin);
        x = (int)fx; y = (int)fy;                           // -1 .. w - 1, -1 .. h - 1
        dx = xin - fx; dy = yin - fy;
        if (UNDO) {                                         // the mask: af_undo_keeps, in place (see there)
            keep = x - 1 >= 0 && x + 2 <= (int)a.w - 1 && y - 1 >= 0 && y + 2 <= (int)a.h - 1;
            for (int k = 0; k < 4 && keep; ++k) {
                double fxin, fyin;
                affine_point(a.fwd, (uint32_t)((k & 1) ? x + 2 : x - 1), (uint32_t)((k & 2) ? y + 2 : y - 1), fxin, fyin);
                keep = affine_inside(fxin, fyin, a.w, a.h);
            }
        }
    }
    if (!keep) {
        dst[0] = other[0]; dst[1] = other[1]; dst[2] = other[2];
        return;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) dst[c] = af_sample<FILTER>(s, x, y, dx, dy, (int)a.w, (int)a.h, c);
}

// The pixels under the mask of an undoing (a.m: the way back, a.fwd: the way there), added to *count.  grid: (tiles across, tiles
// down); block: AFFINE_THREADS; a wave adds its ballot's bits with one atomic
__global__ __launch_bounds__(AFFINE_THREADS) void affine_kept_kernel(AffineArgs a, unsigned long long* __restrict__ count) {
    const uint32_t X = blockIdx.x * AFFINE_TILE_W + threadIdx.x % AFFINE_TILE_W, Y = blockIdx.y * AFFINE_TILE_H + threadIdx.x / AFFINE_TILE_W;
    const bool keep = X < a.w && Y < a.h && af_undo_keeps(a, X, Y);
    const unsigned long long votes = __ballot(keep);
    if ((threadIdx.x & 63) == 0 && votes) atomicAdd(count, (unsigned long long)__popcll(votes));
}

// The undoing of a cut-out of a turned copy (ssw_restore_turned_rgb8): the suspect [h][w][3] laid back into the original's frame
// [oh][ow][3] by a.m (BICUBIC) where the sample point is inside and the footprint needs no clamping, the original's byte elsewhere
// -- one launch, no frame in between.  Under the mask no tap is clamped, so the taps come from global memory as they are.
// grid: (tiles across, tiles down); block: AFFINE_THREADS
__global__ __launch_bounds__(AFFINE_THREADS) void affine_cutout_kernel(AffineArgs a, const uint8_t* __restrict__ in, const uint8_t* __restrict__ base,
                                                                       uint8_t* __restrict__ out) {
    const uint32_t X = blockIdx.x * AFFINE_TILE_W + threadIdx.x % AFFINE_TILE_W, Y = blockIdx.y * AFFINE_TILE_H + threadIdx.x / AFFINE_TILE_W;
    if (X >= a.ow || Y >= a.oh) return;
    const size_t o = ((size_t)Y * a.ow + X) * 3;
    double xin, yin;
    affine_point(a.m, X, Y, xin, yin);
    bool keep = affine_inside(xin, yin, a.w, a.h);          // on the doubles, before any conversion
    int x = 0, y = 0;
    double dx = 0.0, dy = 0.0;
    if (keep) {
        xin -= 0.5; yin -= 0.5;
        const double fx = floor(xin), fy = floor(yin);
        x = (int)fx; y = (int)fy;
        dx = xin - fx; dy = yin - fy;
        keep = x - 1 >= 0 && x + 2 <= (int)a.w - 1 && y - 1 >= 0 && y + 2 <= (int)a.h - 1;
    }
    if (!keep) {
        out[o] = base[o]; out[o + 1] = base[o + 1]; out[o + 2] = base[o + 2];
        return;
    }
    const AffineSource<false> s{in, a.w};
#pragma unroll
    for (int c = 0; c < 3; ++c) out[o + c] = af_sample<AFFINE_BICUBIC>(s, x, y, dx, dy, (int)a.w, (int)a.h, c);
}

namespace host {
namespace {

bool af_side_ok(size_t v) { return v >= 1 && v <= AFFINE_SIDE_MAX; }
bool af_filter_ok(uint32_t f) { return f <= (uint32_t)SSW_AFFINE_BICUBIC; }
bool af_finite(const double* m, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(m[i])) return false;
    return true;
}
bool af_overlaps(const uint8_t* a, size_t na, const uint8_t* b, size_t nb) {
    const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
    return pa < pb + nb && pb < pa + na;
}
bool af_same(const double* a, const double* b, size_t n) { return std::equal(a, a + n, b); }
size_t af_group(size_t fb) { return std::min<size_t>(AFFINE_BATCH, std::max<size_t>(1, AFFINE_GROUP_BYTES / fb)); }

template <int FILTER, bool UNDO>
void af_launch(bool lds, dim3 grid, size_t lds_bytes, hipStream_t st, const AffineFrames& fr, const AffineArgs& a, const uint8_t* in, size_t in_fb,
               const uint8_t* base, uint8_t* out, size_t out_fb) {
    if (lds) affine_kernel<FILTER, true, UNDO><<<grid, AFFINE_THREADS, lds_bytes, st>>>(fr, a, in, in_fb, base, out, out_fb);
    else     affine_kernel<FILTER, false, UNDO><<<grid, AFFINE_THREADS, 0, st>>>(fr, a, in, in_fb, base, out, out_fb);
}

// The launches of one transform: result i [oh][ow][3] at out + i * ow * oh * 3 is frame frames[i] of `in` ([h][w][3], in_fb
// bytes apart) under m; fwd != null: the fused undo over `base` (BICUBIC, ow == w, oh == h)
int affine_enqueue(ssw_ctx* ctx, const uint8_t* in, size_t in_fb, const uint32_t* frames, size_t n, size_t w, size_t h, size_t ow, size_t oh,
                   const double* m, const double* fwd, int filter, const uint8_t* fill, const uint8_t* base, uint8_t* out) {
    const AffinePlan p = affine_plan(m, w, h);
    AffineArgs a{};
    std::copy(m, m + 6, a.m);
    if (fwd) std::copy(fwd, fwd + 6, a.fwd);
    a.w = (uint32_t)w; a.h = (uint32_t)h; a.ow = (uint32_t)ow; a.oh = (uint32_t)oh;
    a.box_w = p.box_w; a.box_h = p.box_h; a.pitch = p.pitch;
    if (fill) std::copy(fill, fill + 3, a.fill);
    const size_t out_fb = ow * oh * 3;
    for (size_t i0 = 0; i0 < n; i0 += AFFINE_BATCH) {
        const unsigned cnt = (unsigned)std::min<size_t>(AFFINE_BATCH, n - i0);
        AffineFrames fr{};
        std::copy(frames + i0, frames + i0 + cnt, fr.src);
        const dim3 grid((unsigned)((ow + AFFINE_TILE_W - 1) / AFFINE_TILE_W), (unsigned)((oh + AFFINE_TILE_H - 1) / AFFINE_TILE_H), cnt);
        uint8_t* o = out + i0 * out_fb;
        if (fwd)                                af_launch<AFFINE_BICUBIC, true>(p.lds, grid, p.lds_bytes, ctx->stream, fr, a, in, in_fb, base, o, out_fb);
        else if (filter == AFFINE_BICUBIC)      af_launch<AFFINE_BICUBIC, false>(p.lds, grid, p.lds_bytes, ctx->stream, fr, a, in, in_fb, base, o, out_fb);
        else                                    af_launch<AFFINE_BILINEAR, false>(p.lds, grid, p.lds_bytes, ctx->stream, fr, a, in, in_fb, base, o, out_fb);
        SSW_HIP_CHECK(hipGetLastError());
    }
    return SSW_OK;
}

bool af_job_is_copy(const ssw_rotate_job& j) { return affine_is_identity(j.forward) && affine_is_identity(j.back); }

}  // namespace

// For the rotation search of angle.hip (ssw_rotate_search_attack_rgb8; ssw_host.hpp declares them): the launches of one
// transform at the frame's own size, and the count of one undoing's mask
int affine_frames(ssw_ctx* ctx, const uint8_t* in, size_t in_fb, const uint32_t* frames, size_t n, size_t w, size_t h, const double* m,
                  const double* fwd, int filter, const uint8_t* fill, const uint8_t* base, uint8_t* out) {
    return affine_enqueue(ctx, in, in_fb, frames, n, w, h, w, h, m, fwd, filter, fill, base, out);
}

int affine_kept_enqueue(ssw_ctx* ctx, size_t w, size_t h, const double* back, const double* forward, unsigned long long* dev_count) {
    const dim3 grid((unsigned)((w + AFFINE_TILE_W - 1) / AFFINE_TILE_W), (unsigned)((h + AFFINE_TILE_H - 1) / AFFINE_TILE_H));
    AffineArgs a{};
    std::copy(back, back + 6, a.m);
    std::copy(forward, forward + 6, a.fwd);
    a.w = a.ow = (uint32_t)w; a.h = a.oh = (uint32_t)h;
    affine_kept_kernel<<<grid, AFFINE_THREADS, 0, ctx->stream>>>(a, dev_count);
    SSW_HIP_CHECK(hipGetLastError());
    return SSW_OK;
}

}  // namespace host
}  // namespace ssw

extern "C" int ssw_affine_plan(size_t w, size_t h, const double* m, int* lds_form, uint32_t* box_w, uint32_t* box_h) {
    if (!m || !lds_form || !ssw::host::af_finite(m, 6)) return SSW_ERR_BAD_ARG;
    if (!ssw::host::af_side_ok(w) || !ssw::host::af_side_ok(h)) return SSW_ERR_BAD_DIMS;
    const ssw::AffinePlan p = ssw::affine_plan(m, w, h);
    *lds_form = p.lds ? 1 : 0;
    if (box_w) *box_w = p.box_w;
    if (box_h) *box_h = p.box_h;
    return SSW_OK;
}

extern "C" int ssw_rotation_matrix(double angle, size_t w, size_t h, double* m) {
    if (!m || !std::isfinite(angle)) return SSW_ERR_BAD_ARG;
    ssw::rotation_matrix(angle, w, h, m);
    return SSW_OK;
}

extern "C" int ssw_affine_rgb8(ssw_ctx* ctx, const uint8_t* dev_in, size_t n_frames, size_t w, size_t h, size_t ow, size_t oh, const double* m,
                               int filter, const uint8_t* fill, uint8_t* dev_out) {
    using namespace ssw::host;
    if (!ctx) return SSW_ERR_BAD_ARG;
    if (n_frames == 0) return SSW_OK;
    if (!dev_in || !dev_out || !m || !fill || filter < 0 || !af_filter_ok((uint32_t)filter) || n_frames > 0xFFFFFFFFull) return SSW_ERR_BAD_ARG;
    if (!af_side_ok(w) || !af_side_ok(h) || !af_side_ok(ow) || !af_side_ok(oh)) return SSW_ERR_BAD_DIMS;
    if (!af_finite(m, 6) || af_overlaps(dev_in, n_frames * w * h * 3, dev_out, n_frames * ow * oh * 3)) return SSW_ERR_BAD_ARG;
    CtxGuard g(ctx);
    StageTimer t(ctx, SSW_STAGE_CONVERT, ctx->stream, (double)n_frames * 3.0 * ((double)w * h + (double)ow * oh));
    std::vector<uint32_t> frames(n_frames);
    for (size_t i = 0; i < n_frames; ++i) frames[i] = (uint32_t)i;
    return affine_enqueue(ctx, dev_in, w * h * 3, frames.data(), n_frames, w, h, ow, oh, m, nullptr, filter, fill, nullptr, dev_out);
}

extern "C" int ssw_rotate_attack_rgb8(ssw_ctx* ctx, const uint8_t* dev_base, const uint8_t* dev_frames, size_t n_frames, size_t w, size_t h,
                                      const ssw_rotate_job* jobs, size_t n_jobs, uint8_t* dev_out) {
    using namespace ssw::host;
    if (!ctx) return SSW_ERR_BAD_ARG;
    if (n_jobs == 0) return SSW_OK;
    if (!dev_base || !dev_frames || !jobs || !dev_out) return SSW_ERR_BAD_ARG;
    if (!af_side_ok(w) || !af_side_ok(h)) return SSW_ERR_BAD_DIMS;
    for (size_t i = 0; i < n_jobs; ++i)
        if (jobs[i].frame >= n_frames || !af_filter_ok(jobs[i].filter) || !af_finite(jobs[i].forward, 6) || !af_finite(jobs[i].back, 6)) return SSW_ERR_BAD_ARG;
    const size_t fb = w * h * 3;
    if (af_overlaps(dev_frames, n_frames * fb, dev_out, n_jobs * fb) || af_overlaps(dev_base, fb, dev_out, n_jobs * fb)) return SSW_ERR_BAD_ARG;
    CtxGuard g(ctx);
    const size_t per = af_group(fb);
    uint8_t* ws = nullptr;
    // groups: consecutive jobs of one filter, fill and pair of matrices, at most `per`: attacked into the workspace, undone from it
    for (size_t j0 = 0; j0 < n_jobs;) {
        const ssw_rotate_job& j = jobs[j0];
        size_t j1 = j0 + 1;
        while (j1 < n_jobs && j1 - j0 < per && jobs[j1].filter == j.filter && std::equal(j.fill, j.fill + 3, jobs[j1].fill) &&
               af_same(jobs[j1].forward, j.forward, 6) && af_same(jobs[j1].back, j.back, 6)) ++j1;
        const size_t cnt = j1 - j0;
        if (af_job_is_copy(j)) {
            StageTimer t(ctx, SSW_STAGE_CONVERT, ctx->stream, (double)cnt * 2.0 * (double)fb);
            for (size_t i = j0; i < j1; ++i)
                SSW_HIP_CHECK(hipMemcpyAsync(dev_out + i * fb, dev_frames + (size_t)jobs[i].frame * fb, fb, hipMemcpyDeviceToDevice, ctx->stream));
            j0 = j1;
            continue;
        }
        if (!ws) SSW_TRY(grow_as(ctx->shared.affine, std::min(per, n_jobs) * fb, ws));
        std::vector<uint32_t> frames(cnt), own(cnt);
        for (size_t i = 0; i < cnt; ++i) { frames[i] = jobs[j0 + i].frame; own[i] = (uint32_t)i; }
        {
            StageTimer t(ctx, SSW_STAGE_CONVERT, ctx->stream, (double)cnt * 2.0 * (double)fb);
            SSW_TRY(affine_enqueue(ctx, dev_frames, fb, frames.data(), cnt, w, h, w, h, j.forward, nullptr, (int)j.filter, j.fill, nullptr, ws));
        }
        {
            StageTimer t(ctx, SSW_STAGE_RESIZE, ctx->stream, (double)cnt * 2.0 * (double)fb);
            SSW_TRY(affine_enqueue(ctx, ws, fb, own.data(), cnt, w, h, w, h, j.back, j.forward, ssw::AFFINE_BICUBIC, nullptr, dev_base, dev_out + j0 * fb));
        }
        j0 = j1;
    }
    return SSW_OK;
}

extern "C" int ssw_unrotate_kept(ssw_ctx* ctx, size_t w, size_t h, const ssw_rotate_job* jobs, size_t n, uint64_t* host_kept) {
    using namespace ssw::host;
    if (!ctx) return SSW_ERR_BAD_ARG;
    if (n == 0) return SSW_OK;
    if (!jobs || !host_kept) return SSW_ERR_BAD_ARG;
    if (!af_side_ok(w) || !af_side_ok(h)) return SSW_ERR_BAD_DIMS;
    for (size_t i = 0; i < n; ++i)
        if (!af_finite(jobs[i].forward, 6) || !af_finite(jobs[i].back, 6)) return SSW_ERR_BAD_ARG;
    CtxGuard g(ctx);
    unsigned long long* dev = nullptr;
    SSW_TRY(grow_as(ctx->shared.affine, n * sizeof(unsigned long long), dev));
    SSW_HIP_CHECK(hipMemsetAsync(dev, 0, n * sizeof(unsigned long long), ctx->stream));
    untimed_work(ctx);
    const dim3 grid((unsigned)((w + ssw::AFFINE_TILE_W - 1) / ssw::AFFINE_TILE_W), (unsigned)((h + ssw::AFFINE_TILE_H - 1) / ssw::AFFINE_TILE_H));
    for (size_t i = 0; i < n; ++i) {
        if (af_job_is_copy(jobs[i])) continue;
        ssw::AffineArgs a{};
        std::copy(jobs[i].back, jobs[i].back + 6, a.m);
        std::copy(jobs[i].forward, jobs[i].forward + 6, a.fwd);
        a.w = a.ow = (uint32_t)w; a.h = a.oh = (uint32_t)h;
        ssw::affine_kept_kernel<<<grid, ssw::AFFINE_THREADS, 0, ctx->stream>>>(a, dev + i);
        SSW_HIP_CHECK(hipGetLastError());
    }
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the counters come down as they are");
    SSW_TRY(download(ctx, host_kept, dev, n * sizeof(uint64_t), ctx->stream));
    for (size_t i = 0; i < n; ++i)
        if (af_job_is_copy(jobs[i])) host_kept[i] = (uint64_t)w * h;
    return SSW_OK;
}

extern "C" int ssw_unrotate_rgb8(ssw_ctx* ctx, const uint8_t* dev_base, const uint8_t* dev_suspects, size_t n, size_t w, size_t h,
                                 const ssw_rotate_job* jobs, uint8_t* dev_out) {
    using namespace ssw::host;
    if (!ctx) return SSW_ERR_BAD_ARG;
    if (n == 0) return SSW_OK;
    if (!dev_base || !dev_suspects || !jobs || !dev_out) return SSW_ERR_BAD_ARG;
    if (!af_side_ok(w) || !af_side_ok(h)) return SSW_ERR_BAD_DIMS;
    for (size_t i = 0; i < n; ++i)
        if (jobs[i].frame >= n || !af_finite(jobs[i].forward, 6) || !af_finite(jobs[i].back, 6)) return SSW_ERR_BAD_ARG;
    const size_t fb = w * h * 3;
    if (af_overlaps(dev_suspects, n * fb, dev_out, n * fb) || af_overlaps(dev_base, fb, dev_out, n * fb)) return SSW_ERR_BAD_ARG;
    CtxGuard g(ctx);
    StageTimer t(ctx, SSW_STAGE_RESIZE, ctx->stream, (double)n * 2.0 * (double)fb);
    for (size_t j0 = 0; j0 < n;) {
        const ssw_rotate_job& j = jobs[j0];
        size_t j1 = j0 + 1;
        while (j1 < n && af_same(jobs[j1].forward, j.forward, 6) && af_same(jobs[j1].back, j.back, 6)) ++j1;
        if (af_job_is_copy(j)) {
            for (size_t i = j0; i < j1; ++i)
                SSW_HIP_CHECK(hipMemcpyAsync(dev_out + i * fb, dev_suspects + (size_t)jobs[i].frame * fb, fb, hipMemcpyDeviceToDevice, ctx->stream));
        } else {
            std::vector<uint32_t> frames(j1 - j0);
            for (size_t i = j0; i < j1; ++i) frames[i - j0] = jobs[i].frame;
            SSW_TRY(affine_enqueue(ctx, dev_suspects, fb, frames.data(), j1 - j0, w, h, w, h, j.back, j.forward, ssw::AFFINE_BICUBIC, nullptr, dev_base,
                                   dev_out + j0 * fb));
        }
        j0 = j1;
    }
    return SSW_OK;
}

extern "C" int ssw_restore_turned_rgb8(ssw_ctx* ctx, const uint8_t* dev_base, size_t w, size_t h, const void* const* dev_suspects,
                                       const ssw_turned_shape* shapes, const ssw_turned_job* jobs, size_t n, uint8_t* dev_out) {
    using namespace ssw::host;
    if (!ctx) return SSW_ERR_BAD_ARG;
    if (n == 0) return SSW_OK;
    if (!dev_base || !dev_suspects || !shapes || !jobs || !dev_out) return SSW_ERR_BAD_ARG;
    for (size_t i = 0; i < n; ++i)
        if (!dev_suspects[i] || (shapes[i].channels != 3 && shapes[i].channels != 4) || !std::isfinite(jobs[i].angle) || !std::isfinite(jobs[i].cx) ||
            !std::isfinite(jobs[i].cy)) return SSW_ERR_BAD_ARG;
    if (!af_side_ok(w) || !af_side_ok(h)) return SSW_ERR_BAD_DIMS;
    for (size_t i = 0; i < n; ++i)
        if (!af_side_ok(shapes[i].w) || !af_side_ok(shapes[i].h)) return SSW_ERR_BAD_DIMS;
    const size_t fb = w * h * 3;
    for (size_t i = 0; i < n; ++i) {
        if (shapes[i].channels == 4) return SSW_ERR_UNSUPPORTED;
        if (af_overlaps((const uint8_t*)dev_suspects[i], (size_t)shapes[i].w * shapes[i].h * 3, dev_out, n * fb)) return SSW_ERR_BAD_ARG;
    }
    if (af_overlaps(dev_base, fb, dev_out, n * fb)) return SSW_ERR_BAD_ARG;
    CtxGuard g(ctx);
    double bytes = 0.0;
    for (size_t i = 0; i < n; ++i) bytes += 3.0 * (double)shapes[i].w * shapes[i].h + (double)fb;
    StageTimer t(ctx, SSW_STAGE_RESIZE, ctx->stream, bytes);
    const dim3 grid((unsigned)((w + ssw::AFFINE_TILE_W - 1) / ssw::AFFINE_TILE_W), (unsigned)((h + ssw::AFFINE_TILE_H - 1) / ssw::AFFINE_TILE_H));
    for (size_t i = 0; i < n; ++i) {
        ssw::AffineArgs a{};
        ssw::turned_restore_matrix(jobs[i].angle, jobs[i].cx, jobs[i].cy, shapes[i].w, shapes[i].h, a.m);
        if (!af_finite(a.m, 6)) return SSW_ERR_BAD_ARG;
        a.w = shapes[i].w; a.h = shapes[i].h; a.ow = (uint32_t)w; a.oh = (uint32_t)h;
        ssw::affine_cutout_kernel<<<grid, ssw::AFFINE_THREADS, 0, ctx->stream>>>(a, (const uint8_t*)dev_suspects[i], dev_base, dev_out + i * fb);
        SSW_HIP_CHECK(hipGetLastError());
    }
    return SSW_OK;
}
