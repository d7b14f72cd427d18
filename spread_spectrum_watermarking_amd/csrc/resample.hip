// The scale attack (ssw_resample_rgb8, ssw_scale_attack_rgb8): a marked copy as PIL.Image.resize makes its thumbnail, and that
// thumbnail brought back to the original's size the way ssw_restore_rgb8 brings back a suspect of another size.  include/ssw.h
// states the definition; it is Pillow's 8-bit resample (Resample.c), integer arithmetic on the bytes with 22-bit fixed-point
// taps, so the frames equal the numpy restatement of tests/test_resample_cpu.py -- and with it Pillow -- exactly.  The reference
// has no counterpart.
//
// Two kernels with Pillow's own structure (grid z: the frames of a launch, RS_BATCH at most, their indices as kernel arguments):
//   resample_rows_kernel<true>   a block takes RS_ROWS rows and a run of output columns.  The run's left / count / taps go to LDS,
//                       tap-major (tap t of column c at t * run + c), so that the lanes of a wave, three to a column, read
//                       consecutive words; the contiguous input span of the run goes to LDS as bytes, loaded as dwords at
//                       whatever alignment the frame has.  A thread takes one output byte at a time, consecutive lanes consecutive
//                       bytes of a row: count multiply-adds of a 24-bit tap and a byte (the 24-bit multiply applies), rounded,
//                       clamped and stored to the byte plane [h][nw][3] -- a wave's 64 stores are one contiguous run.  The host
//                       sizes the run from the LDS that is left (resample_rows_plan).
//   resample_rows_kernel<false>  the same arithmetic with taps and samples read from global memory: the form for ratios at which
//                       not even a run of 4 columns fits (a 4K row reduced to 7 columns by LANCZOS spans 3291 pixels a column).
//   resample_cols_kernel         the plane as an h x 3 nw matrix of bytes: a thread owns one byte column of an output row and
//                       walks its taps down the plane, four rows a step -- the four bytes are loaded first, then multiplied; the
//                       table is padded with zero taps to a multiple of four and the row index is clamped, so no load sits behind
//                       a branch.  The taps of a row are uniform over the block.
// A pass whose length does not change is skipped: the other kernel then reads the frame or writes the result itself.  The tables
// of a call are made on the host (resample_tables.hpp) and go up in one copy on the stream, into the workspace beside the plane.
// Neither kernel assumes any alignment of a pointer or of a row.
#include <algorithm>
#include <vector>

#include "resample_tables.hpp"
#include "ssw_host.hpp"

namespace ssw {

constexpr unsigned RS_BATCH = 32;                       // frames per launch
constexpr size_t RS_GROUP_BYTES = (size_t)64 << 20;     // planes (and thumbnails) kept at a time (one frame's, if it is larger)
constexpr size_t RS_SIDE_MAX = 65535;
constexpr unsigned RS_ROWS = 8;                         // rows of a block of the row kernel
constexpr unsigned RS_RUN_MAX = 256, RS_RUN_MIN = 4;    // output columns of a block of the row kernel
constexpr size_t RS_LDS_BYTES = 64 << 10;
constexpr int RS_HALF = 1 << (RESAMPLE_BITS - 1);

struct ResampleFrames { uint32_t src[RS_BATCH]; };      // the frame of the input that result z of the launch is made of
struct ResampleAxis { const uint32_t* left; const uint32_t* count; const int32_t* taps; uint32_t kstride; };

__device__ inline uint32_t rs_clip8(int v) { return (uint32_t)min(max(v >> RESAMPLE_BITS, 0), 255); }

// one output byte: n taps `tstride` words apart against the samples of its channel, 3 bytes apart from p on
__device__ inline uint8_t rs_sample(const uint8_t* __restrict__ p, const int32_t* __restrict__ tap, unsigned tstride, unsigned n) {
    int a = RS_HALF;
    for (unsigned t = 0; t < n; ++t) a += __mul24(tap[t * tstride], (int)p[3 * t]);
    return (uint8_t)rs_clip8(a);
}

// grid: (runs of `run` output columns, bands of RS_ROWS rows, frames of the launch); block: 256.  in: frames [h][w][3] `in_fb`
// bytes apart; out: [z][h][nw][3], `out_fb` bytes apart.  ax.taps: [kmax][nw].  LDS form: `pitch` bytes a staged row (a multiple
// of 4, at least the longest span of a run); dynamic LDS (2 + kmax) * run words + RS_ROWS * pitch bytes.
template <bool LDS>
__global__ __launch_bounds__(256) void resample_rows_kernel(ResampleFrames fr, const uint8_t* __restrict__ in, size_t in_fb, uint32_t w, uint32_t h,
                                                            uint32_t nw, ResampleAxis ax, uint32_t kmax, uint32_t run, uint32_t pitch,
                                                            uint8_t* __restrict__ out, size_t out_fb) {
    extern __shared__ __attribute__((aligned(16))) uint32_t rs_smem[];
    const unsigned t = threadIdx.x;
    const unsigned c0 = blockIdx.x * run, nc = min(run, nw - c0);
    const unsigned y0 = blockIdx.y * RS_ROWS, rows = min(RS_ROWS, h - y0);
    const size_t row_bytes = (size_t)w * 3;
    const uint8_t* __restrict__ src = in + (size_t)fr.src[blockIdx.z] * in_fb + (size_t)y0 * row_bytes;
    uint8_t* __restrict__ dst = out + (size_t)blockIdx.z * out_fb + ((size_t)y0 * nw + c0) * 3;
    if (LDS) {
        uint32_t* s_left = rs_smem;
        uint32_t* s_count = rs_smem + run;
        int32_t* s_taps = reinterpret_cast<int32_t*>(rs_smem + 2 * run);
        uint8_t* s_px = reinterpret_cast<uint8_t*>(rs_smem + (size_t)(2 + kmax) * run);
        const unsigned x_lo = ax.left[c0], x_hi = ax.left[c0 + nc - 1] + ax.count[c0 + nc - 1];      // left and left + count never decrease
        const unsigned span = 3 * (x_hi - x_lo), dwords = span / 4, tail = span - 4 * dwords;
        for (unsigned i = t; i < nc; i += 256) { s_left[i] = ax.left[c0 + i] - x_lo; s_count[i] = ax.count[c0 + i]; }
        for (unsigned i = t; i < kmax * nc; i += 256) {
            const unsigned k = i / nc, c = i - k * nc;
            s_taps[k * run + c] = ax.taps[(size_t)k * nw + c0 + c];
        }
        const uint8_t* __restrict__ sp = src + (size_t)x_lo * 3;
        for (unsigned i = t; i < rows * dwords; i += 256) {
            const unsigned r = i / dwords, d = i - r * dwords;
            uint32_t v;
            __builtin_memcpy(&v, sp + r * row_bytes + 4 * d, 4);
            *reinterpret_cast<uint32_t*>(s_px + r * pitch + 4 * d) = v;
        }
        for (unsigned i = t; i < rows * tail; i += 256) {
            const unsigned r = i / tail, j = 4 * dwords + (i - r * tail);
            s_px[r * pitch + j] = sp[r * row_bytes + j];
        }
        __syncthreads();
        for (unsigned i = t; i < rows * nc * 3; i += 256) {                 // consecutive lanes: consecutive bytes of an output row
            const unsigned r = i / (nc * 3), b = i - r * nc * 3, c = b / 3;
            dst[(size_t)r * nw * 3 + b] = rs_sample(s_px + r * pitch + 3 * s_left[c] + (b - 3 * c), s_taps + c, run, s_count[c]);
        }
    } else {
        for (unsigned i = t; i < rows * nc * 3; i += 256) {
            const unsigned r = i / (nc * 3), b = i - r * nc * 3, c = b / 3;
            dst[(size_t)r * nw * 3 + b] = rs_sample(src + r * row_bytes + (size_t)ax.left[c0 + c] * 3 + (b - 3 * c), ax.taps + c0 + c, nw, ax.count[c0 + c]);
        }
    }
}

// grid: (groups of 256 bytes of a row, output rows, frames of the launch); block: 256.  in: planes [h][row_bytes] `in_fb` bytes
// apart, plane z for result z unless `direct` (then frame fr.src[z] of the call's input: the row pass was skipped).
// ax.taps: [nh][kstride], kstride a multiple of 4, zero beyond count.  A thread owns one byte column of the output row: a wave's
// loads and stores are 64 consecutive bytes.
__global__ __launch_bounds__(256) void resample_cols_kernel(ResampleFrames fr, uint32_t direct, const uint8_t* __restrict__ in, size_t in_fb,
                                                            uint32_t row_bytes, uint32_t h, ResampleAxis ax, uint8_t* __restrict__ out, size_t out_fb) {
    const unsigned b = blockIdx.x * 256 + threadIdx.x;
    if (b >= row_bytes) return;
    const unsigned y = blockIdx.y, top = ax.left[y], n = ax.count[y];
    const int32_t* __restrict__ tap = ax.taps + (size_t)y * ax.kstride;
    const uint8_t* __restrict__ src = in + (size_t)(direct ? fr.src[blockIdx.z] : blockIdx.z) * in_fb + b;
    int a = RS_HALF;
    for (unsigned t = 0; t < n; t += 4) {
        int v[4];
#pragma unroll
        for (unsigned j = 0; j < 4; ++j) v[j] = (int)src[(size_t)min(top + t + j, h - 1) * row_bytes];
#pragma unroll
        for (unsigned j = 0; j < 4; ++j) a += __mul24(tap[t + j], v[j]);
    }
    out[(size_t)blockIdx.z * out_fb + (size_t)y * row_bytes + b] = (uint8_t)rs_clip8(a);
}

namespace host {
namespace {

// One (w, h) -> (nw, nh) resample with one filter: the host tables, their device image (one blob of words: left | count | taps
// of the row pass, tap-major; the same of the column pass, taps row-major with a stride that is a multiple of 4), the row
// kernel's run and the bytes of the plane of one frame.
struct ResamplePlan {
    size_t w = 0, h = 0, nw = 0, nh = 0;
    int filter = 0;
    bool rows = false, cols = false;        // which passes run
    ResampleTable th, tv;
    bool lds = false;
    uint32_t run = RS_RUN_MIN, pitch = 4, kstride = 4;
    size_t lds_bytes = 0;
    std::vector<uint32_t> blob;
    size_t off_h = 0, off_v = 0;            // words
    size_t plane_fb() const { return rows && cols ? h * nw * 3 : 0; }
    size_t table_bytes() const { return (blob.size() * 4 + 255) & ~(size_t)255; }
    size_t group() const { return std::min<size_t>(RS_BATCH, plane_fb() ? std::max<size_t>(1, RS_GROUP_BYTES / plane_fb()) : RS_BATCH); }
    size_t workspace() const { return table_bytes() + group() * plane_fb(); }
};

// the largest run of output columns whose tables and staged rows fit RS_LDS_BYTES; false: not even RS_RUN_MIN do
bool resample_rows_plan(const ResampleTable& t, size_t out_len, uint32_t* run, uint32_t* pitch, size_t* lds) {
    for (size_t c = 1; c < out_len; ++c)
        if (t.left[c] < t.left[c - 1] || t.left[c] + t.count[c] < t.left[c - 1] + t.count[c - 1]) return false;
    uint32_t first = RS_RUN_MAX;                            // no wider than the axis needs
    while (first > RS_RUN_MIN && first / 2 >= out_len) first /= 2;
    for (uint32_t r = first; r >= RS_RUN_MIN; r /= 2) {
        size_t span = 0;
        for (size_t c0 = 0; c0 < out_len; c0 += r) {
            const size_t last = std::min<size_t>(c0 + r, out_len) - 1;
            span = std::max<size_t>(span, (size_t)t.left[last] + t.count[last] - t.left[c0]);
        }
        const size_t p = (3 * span + 3) & ~(size_t)3;
        const size_t bytes = (size_t)(2 + t.kmax) * r * 4 + RS_ROWS * std::max<size_t>(p, 4);
        if (bytes <= RS_LDS_BYTES) { *run = r; *pitch = (uint32_t)std::max<size_t>(p, 4); *lds = bytes; return true; }
    }
    return false;
}

// false: a tap that does not fit 24 bits signed (none of the four filters makes one: a normalised weight stays below 2)
bool resample_plan(size_t w, size_t h, size_t nw, size_t nh, int filter, ResamplePlan& p) {
    p.w = w; p.h = h; p.nw = nw; p.nh = nh; p.filter = filter;
    p.rows = nw != w; p.cols = nh != h;
    p.blob.clear();
    if (p.rows) {
        build_resample_table(w, nw, filter, p.th);
        p.lds = resample_rows_plan(p.th, nw, &p.run, &p.pitch, &p.lds_bytes);
        if (!p.lds) { p.run = 64; p.pitch = 4; p.lds_bytes = 0; }
        p.off_h = 0;
        p.blob.insert(p.blob.end(), p.th.left.begin(), p.th.left.end());
        p.blob.insert(p.blob.end(), p.th.count.begin(), p.th.count.end());
        const size_t at = p.blob.size();
        p.blob.resize(at + (size_t)p.th.kmax * nw);
        for (size_t c = 0; c < nw; ++c)
            for (size_t k = 0; k < p.th.kmax; ++k) p.blob[at + k * nw + c] = (uint32_t)p.th.taps[c * p.th.kmax + k];
    }
    if (p.cols) {
        build_resample_table(h, nh, filter, p.tv);
        p.kstride = (p.tv.kmax + 3) & ~3u;
        p.off_v = p.blob.size();
        p.blob.insert(p.blob.end(), p.tv.left.begin(), p.tv.left.end());
        p.blob.insert(p.blob.end(), p.tv.count.begin(), p.tv.count.end());
        const size_t at = p.blob.size();
        p.blob.resize(at + (size_t)p.kstride * nh, 0u);
        for (size_t y = 0; y < nh; ++y)
            for (size_t k = 0; k < p.tv.kmax; ++k) p.blob[at + y * p.kstride + k] = (uint32_t)p.tv.taps[y * p.tv.kmax + k];
    }
    for (const ResampleTable* t : {&p.th, &p.tv})
        for (int32_t v : t->taps)
            if (v <= -(1 << 23) || v >= (1 << 23)) return false;
    return true;
}

double resample_work(const ResamplePlan& p) {
    return 3.0 * ((double)p.w * p.h + (double)p.nw * p.nh) + (p.rows && p.cols ? 6.0 * (double)p.nw * p.h : 0.0);
}

// The launches of one plan: result i [nh][nw][3] at out + i * nw * nh * 3 is frame frames[i] of `in`.  ws: the plan's
// workspace() bytes, the tables first.  The tables go up once, on the stream (a pageable source: the runtime has taken the bytes
// when the copy call returns, as with the tap tables of ssw_resize_rgb8).
int resample_enqueue(ssw_ctx* ctx, const ResamplePlan& p, uint8_t* ws, bool tables_up, const uint8_t* in, const uint32_t* frames, size_t n, uint8_t* out) {
    hipStream_t st = ctx->stream;
    if (!tables_up) SSW_HIP_CHECK(hipMemcpyAsync(ws, p.blob.data(), p.blob.size() * 4, hipMemcpyHostToDevice, st));
    const uint32_t* words = reinterpret_cast<const uint32_t*>(ws);
    const ResampleAxis ah{words + p.off_h, words + p.off_h + p.nw, reinterpret_cast<const int32_t*>(words + p.off_h + 2 * p.nw), p.th.kmax};
    const ResampleAxis av{words + p.off_v, words + p.off_v + p.nh, reinterpret_cast<const int32_t*>(words + p.off_v + 2 * p.nh), p.kstride};
    uint8_t* planes = ws + p.table_bytes();
    const size_t in_fb = p.w * p.h * 3, out_fb = p.nw * p.nh * 3, plane_fb = p.plane_fb(), group = p.group();
    const uint32_t W = (uint32_t)p.w, H = (uint32_t)p.h, NW = (uint32_t)p.nw, NH = (uint32_t)p.nh;
    for (size_t i0 = 0; i0 < n; i0 += group) {
        const unsigned m = (unsigned)std::min(group, n - i0);
        ResampleFrames fr{};
        std::copy(frames + i0, frames + i0 + m, fr.src);
        uint8_t* o = out + i0 * out_fb;
        if (p.rows) {
            uint8_t* to = p.cols ? planes : o;
            const size_t to_fb = p.cols ? plane_fb : out_fb;
            const dim3 grid((NW + p.run - 1) / p.run, (H + RS_ROWS - 1) / RS_ROWS, m);
            if (p.lds) resample_rows_kernel<true><<<grid, 256, p.lds_bytes, st>>>(fr, in, in_fb, W, H, NW, ah, p.th.kmax, p.run, p.pitch, to, to_fb);
            else       resample_rows_kernel<false><<<grid, 256, 0, st>>>(fr, in, in_fb, W, H, NW, ah, p.th.kmax, p.run, p.pitch, to, to_fb);
            SSW_HIP_CHECK(hipGetLastError());
        }
        if (p.cols) {
            const uint32_t row_bytes = NW * 3;
            const dim3 grid((row_bytes + 255) / 256, NH, m);
            resample_cols_kernel<<<grid, 256, 0, st>>>(fr, p.rows ? 0u : 1u, p.rows ? planes : in, p.rows ? plane_fb : in_fb, row_bytes, H, av, o, out_fb);
            SSW_HIP_CHECK(hipGetLastError());
        }
    }
    return SSW_OK;
}

bool side_ok(size_t v) { return v >= 1 && v <= RS_SIDE_MAX; }
bool filter_ok(uint32_t f) { return f <= (uint32_t)SSW_RESAMPLE_LANCZOS; }
bool overlaps(const uint8_t* a, size_t na, const uint8_t* b, size_t nb) {
    const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
    return pa < pb + nb && pb < pa + na;
}

}  // namespace
}  // namespace host
}  // namespace ssw

extern "C" int ssw_resample_rgb8(ssw_ctx* ctx, const uint8_t* dev_in, size_t n_frames, size_t w, size_t h, size_t nw, size_t nh, int filter,
                                 uint8_t* dev_out) {
    using namespace ssw::host;
    if (!ctx) return SSW_ERR_BAD_ARG;
    if (n_frames == 0) return SSW_OK;
    if (!dev_in || !dev_out || filter < 0 || !filter_ok((uint32_t)filter) || n_frames > 0xFFFFFFFFull) return SSW_ERR_BAD_ARG;
    if (!side_ok(w) || !side_ok(h) || !side_ok(nw) || !side_ok(nh)) return SSW_ERR_BAD_DIMS;
    if (overlaps(dev_in, n_frames * w * h * 3, dev_out, n_frames * nw * nh * 3)) return SSW_ERR_BAD_ARG;
    CtxGuard g(ctx);
    ResamplePlan p;
    if (!resample_plan(w, h, nw, nh, filter, p)) return SSW_ERR_UNSUPPORTED;
    StageTimer t(ctx, SSW_STAGE_CONVERT, ctx->stream, (double)n_frames * resample_work(p));
    if (!p.rows && !p.cols) {
        SSW_HIP_CHECK(hipMemcpyAsync(dev_out, dev_in, n_frames * w * h * 3, hipMemcpyDeviceToDevice, ctx->stream));
        return SSW_OK;
    }
    SSW_TRY(grow(ctx->shared.resample, p.workspace()));
    std::vector<uint32_t> frames(n_frames);
    for (size_t i = 0; i < n_frames; ++i) frames[i] = (uint32_t)i;
    return resample_enqueue(ctx, p, ctx->shared.resample.as<uint8_t>(), false, dev_in, frames.data(), n_frames, dev_out);
}

extern "C" int ssw_scale_attack_rgb8(ssw_ctx* ctx, const uint8_t* dev_frames, size_t n_frames, size_t w, size_t h, const ssw_scale_job* jobs,
                                     size_t n_jobs, uint8_t* dev_out) {
    using namespace ssw::host;
    if (!ctx) return SSW_ERR_BAD_ARG;
    if (n_jobs == 0) return SSW_OK;
    if (!dev_frames || !jobs || !dev_out) return SSW_ERR_BAD_ARG;
    if (!side_ok(w) || !side_ok(h)) return SSW_ERR_BAD_DIMS;
    for (size_t i = 0; i < n_jobs; ++i) {
        if (jobs[i].frame >= n_frames || !filter_ok(jobs[i].filter)) return SSW_ERR_BAD_ARG;
        if (!side_ok(jobs[i].nw) || !side_ok(jobs[i].nh)) return SSW_ERR_BAD_DIMS;
    }
    const size_t fb = w * h * 3;
    if (overlaps(dev_frames, n_frames * fb, dev_out, n_jobs * fb)) return SSW_ERR_BAD_ARG;
    CtxGuard g(ctx);

    // batches: consecutive jobs of one (nw, nh, filter).  Every plan and every tap table of the way back is made before anything
    // is enqueued; the workspace is sized for the largest batch: tables | planes | thumbnails
    struct Batch { size_t j0, j1; bool copy; ResamplePlan plan; size_t per; };
    std::vector<Batch> batches;
    for (size_t j0 = 0; j0 < n_jobs;) {
        size_t j1 = j0 + 1;
        while (j1 < n_jobs && jobs[j1].nw == jobs[j0].nw && jobs[j1].nh == jobs[j0].nh && jobs[j1].filter == jobs[j0].filter) ++j1;
        batches.emplace_back();
        Batch& b = batches.back();
        b.j0 = j0; b.j1 = j1; b.copy = jobs[j0].nw == w && jobs[j0].nh == h; b.per = 0;
        j0 = j1;
    }
    size_t front = 0, thumbs = 0;
    for (Batch& b : batches) {
        if (b.copy) continue;
        const ssw_scale_job& j = jobs[b.j0];
        if (!resample_plan(w, h, j.nw, j.nh, (int)j.filter, b.plan)) return SSW_ERR_UNSUPPORTED;
        const size_t tfb = (size_t)j.nw * j.nh * 3;
        b.per = std::min(b.j1 - b.j0, std::max<size_t>(1, ssw::RS_GROUP_BYTES / tfb));
        front = std::max(front, b.plan.workspace());
        thumbs = std::max(thumbs, b.per * tfb);
        const std::vector<ssw_placement> pl{ssw_placement{j.nw, j.nh, 3, 0, 0, (uint32_t)w, (uint32_t)h}};
        SSW_TRY(restore_prepare(ctx, pl));
    }
    front = (front + 255) & ~(size_t)255;
    if (front + thumbs) SSW_TRY(grow(ctx->shared.resample, front + thumbs));
    uint8_t* ws = ctx->shared.resample.as<uint8_t>();
    for (const Batch& b : batches) {
        if (b.copy) {
            StageTimer t(ctx, SSW_STAGE_CONVERT, ctx->stream, (double)(b.j1 - b.j0) * 2.0 * (double)fb);
            for (size_t i = b.j0; i < b.j1; ++i)
                SSW_HIP_CHECK(hipMemcpyAsync(dev_out + i * fb, dev_frames + (size_t)jobs[i].frame * fb, fb, hipMemcpyDeviceToDevice, ctx->stream));
            continue;
        }
        const ssw_scale_job& j = jobs[b.j0];
        const size_t tfb = (size_t)j.nw * j.nh * 3;
        const ssw_placement pl{j.nw, j.nh, 3, 0, 0, (uint32_t)w, (uint32_t)h};
        for (size_t i0 = b.j0; i0 < b.j1; i0 += b.per) {
            const size_t m = std::min(b.per, b.j1 - i0);
            std::vector<uint32_t> frames(m);
            std::vector<RestoreJob> back(m);
            for (size_t i = 0; i < m; ++i) {
                frames[i] = jobs[i0 + i].frame;
                back[i] = RestoreJob{ws + front + i * tfb, dev_out + (i0 + i) * fb, pl};
            }
            {
                StageTimer t(ctx, SSW_STAGE_CONVERT, ctx->stream, (double)m * resample_work(b.plan));
                SSW_TRY(resample_enqueue(ctx, b.plan, ws, i0 != b.j0, dev_frames, frames.data(), m, ws + front));
            }
            SSW_TRY(restore_enqueue(ctx, nullptr, w, h, back.data(), m));       // a whole-frame placement never reads the original
        }
    }
    return SSW_OK;
}
