// The crop attack of the strength report (ssw_crop_attack_rgb8, ssw_crop_search_attack_rgb8; include/ssw.h states both as
// compositions of ssw_resample_rgb8, ssw_locate_rgb8, ssw_locate_scaled_rgb8 and ssw_restore_rgb8): a rectangle is cut out of
// a marked copy, perhaps made a thumbnail, and laid over the original again -- where the caller says (the reference's test,
// tests/attack_crop.rs:56-70) or where the tracer's own search finds it.
//
// The resizes, the searches and the restore of a resized or searched piece are the older entry points, called as they are:
// this file adds no path through their kernels.  Two kernels are new, both plain byte movers bound by HBM:
//   crop_cut_kernel          the dense piece [ch][cw][3] of a rectangle of a frame (the input of a resize or a search, and the
//                            thumbnail the caller asked for)
//   crop_complement_kernel   the placed, unscaled job in one pass: every output row is the original's bytes, the copy's, the
//                            original's.  No piece is made, so the frame ssw_restore_rgb8 would read back is never written.
// Neither assumes a pitch or an alignment: a row of a rectangle starts at byte 3 x of a row of 3 W bytes, and a frame of odd
// size starts on any byte.  A thread owns one 16-byte ALIGNED chunk of the destination row.  A chunk that lies inside the row
// and inside one source is stored as one 16-byte word whose four words are formed from the (up to five) aligned source words
// that hold its bytes (v_alignbyte_b32 through its builtin): every one of those words holds at least one byte the chunk needs,
// so nothing outside the source is read.  The at most two chunks at a row's ends, and those that straddle an edge of the
// rectangle, go byte by byte, each byte from its own source.  Descriptors travel as kernel arguments, 32 jobs a launch.
#include <algorithm>
#include <vector>

#include "ssw_host.hpp"

namespace ssw {

constexpr unsigned CROP_BATCH = 32;
constexpr size_t CROP_GROUP_BYTES = (size_t)256 << 20;       // pieces and thumbnails of one group of jobs (one job's, if larger)
constexpr size_t CROP_SIDE_MAX = 65535;

struct CropCutDev { const uint8_t* src; uint8_t* dst; uint32_t cw3, ch; };      // src: the rectangle's first byte in its frame
struct CropCutBatch { CropCutDev it[CROP_BATCH]; };
struct CropCompDev { const uint8_t* copy; uint8_t* out; uint32_t x3, cw3, y, ch; };
struct CropCompBatch { CropCompDev it[CROP_BATCH]; };

// 16 bytes from any address: the aligned words that hold them, shifted into place
__device__ inline uint4 crop_load16(const uint8_t* s) {
    const unsigned sh = (unsigned)(reinterpret_cast<uintptr_t>(s) & 3);
    const uint32_t* p = reinterpret_cast<const uint32_t*>(s - sh);
    if (sh == 0) {
        if ((reinterpret_cast<uintptr_t>(p) & 15) == 0) return *reinterpret_cast<const uint4*>(p);
        return make_uint4(p[0], p[1], p[2], p[3]);
    }
    const uint32_t w0 = p[0], w1 = p[1], w2 = p[2], w3 = p[3], w4 = p[4];       // p[4] holds byte 15 of the chunk: sh >= 1
    return make_uint4(__builtin_amdgcn_alignbyte(w1, w0, sh), __builtin_amdgcn_alignbyte(w2, w1, sh),
                      __builtin_amdgcn_alignbyte(w3, w2, sh), __builtin_amdgcn_alignbyte(w4, w3, sh));
}

// One thread = one aligned 16-byte chunk of a piece's row.  grid: (chunks of a row / 256, rows, jobs).
__global__ __launch_bounds__(256) void crop_cut_kernel(unsigned W3, CropCutBatch b) {
    const CropCutDev& d = b.it[blockIdx.z];
    const unsigned k = blockIdx.x * 256 + threadIdx.x;
    for (unsigned row = blockIdx.y; row < d.ch; row += gridDim.y) {
        uint8_t* __restrict__ drow = d.dst + (size_t)row * d.cw3;
        const uint8_t* __restrict__ srow = d.src + (size_t)row * W3;
        const int a = (int)(reinterpret_cast<uintptr_t>(drow) & 15);
        const int c0 = (int)(16 * k) - a, c1 = c0 + 16, n = (int)d.cw3;        // the chunk covers bytes c0 .. c1 - 1 of the row
        if (c0 >= n) continue;
        if (c0 >= 0 && c1 <= n) {
            *reinterpret_cast<uint4*>(drow + c0) = crop_load16(srow + c0);
        } else {
            for (int c = c0 < 0 ? 0 : c0; c < (c1 < n ? c1 : n); ++c) drow[c] = srow[c];
        }
    }
}

// One thread = one aligned 16-byte chunk of a frame's row.  grid: (chunks of a row / 256, rows, jobs).
__global__ __launch_bounds__(256) void crop_complement_kernel(const uint8_t* __restrict__ base, unsigned W3, unsigned H, CropCompBatch b) {
    const CropCompDev& d = b.it[blockIdx.z];
    const unsigned k = blockIdx.x * 256 + threadIdx.x;
    for (unsigned row = blockIdx.y; row < H; row += gridDim.y) {
        const size_t off = (size_t)row * W3;
        uint8_t* __restrict__ drow = d.out + off;
        const uint8_t* __restrict__ orow = base + off;
        const uint8_t* __restrict__ crow = d.copy + off;
        const int a = (int)(reinterpret_cast<uintptr_t>(drow) & 15);
        const int c0 = (int)(16 * k) - a, c1 = c0 + 16, n = (int)W3;
        if (c0 >= n) continue;
        const bool in_row = row >= d.y && row - d.y < d.ch;
        const int lo = in_row ? (int)d.x3 : n, hi = in_row ? (int)(d.x3 + d.cw3) : n;      // the copy's bytes of this row: lo .. hi - 1
        if (c0 >= 0 && c1 <= n && (c1 <= lo || c0 >= hi)) {
            *reinterpret_cast<uint4*>(drow + c0) = crop_load16(orow + c0);
        } else if (c0 >= lo && c1 <= hi) {               // (lo >= 0 and hi <= n: the chunk lies inside the row)
            *reinterpret_cast<uint4*>(drow + c0) = crop_load16(crow + c0);
        } else {
            for (int c = c0 < 0 ? 0 : c0; c < (c1 < n ? c1 : n); ++c) drow[c] = (c >= lo && c < hi) ? crow[c] : orow[c];
        }
    }
}

namespace host {

namespace {

bool overlaps(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
    return na && nb && pa < pb + nb && pb < pa + na;
}

bool scaled(const ssw_crop_job& j) { return j.tw != 0; }
size_t piece_bytes(const ssw_crop_job& j) { return (size_t)j.cw * j.ch * 3; }
size_t thumb_bytes(const ssw_crop_job& j) { return scaled(j) ? (size_t)j.tw * j.th * 3 : piece_bytes(j); }
bool same_class(const ssw_crop_job& a, const ssw_crop_job& b) {
    return a.cw == b.cw && a.ch == b.ch && a.tw == b.tw && a.th == b.th && a.filter == b.filter;
}

int crop_check(const ssw_ctx* ctx, const uint8_t* dev_base, const uint8_t* dev_frames, size_t n_frames, size_t w, size_t h,
               const ssw_crop_job* jobs, size_t n_jobs, const uint8_t* dev_out, const uint8_t* dev_thumbs, size_t* thumbs_total) {
    if (!dev_base || !dev_frames || !jobs || !dev_out) return SSW_ERR_BAD_ARG;
    if (w == 0 || h == 0 || w > CROP_SIDE_MAX || h > CROP_SIDE_MAX) return SSW_ERR_BAD_DIMS;
    size_t total = 0;
    for (size_t i = 0; i < n_jobs; ++i) {
        const ssw_crop_job& j = jobs[i];
        if (j.frame >= n_frames || j.cw == 0 || j.ch == 0 || (j.tw == 0) != (j.th == 0)) return SSW_ERR_BAD_ARG;
        if ((uint64_t)j.x + j.cw > w || (uint64_t)j.y + j.ch > h) return SSW_ERR_BAD_ARG;
        if (scaled(j) && j.filter > (uint32_t)SSW_RESAMPLE_LANCZOS) return SSW_ERR_BAD_ARG;
        if (j.tw > CROP_SIDE_MAX || j.th > CROP_SIDE_MAX) return SSW_ERR_BAD_DIMS;
        total += thumb_bytes(j);
    }
    const size_t fb = w * h * 3;
    if (overlaps(dev_out, n_jobs * fb, dev_frames, n_frames * fb) || overlaps(dev_out, n_jobs * fb, dev_base, fb)) return SSW_ERR_BAD_ARG;
    if (dev_thumbs && (overlaps(dev_thumbs, total, dev_frames, n_frames * fb) || overlaps(dev_thumbs, total, dev_base, fb) ||
                       overlaps(dev_thumbs, total, dev_out, n_jobs * fb))) return SSW_ERR_BAD_ARG;
    *thumbs_total = total;
    (void)ctx;
    return SSW_OK;
}

int cut_enqueue(ssw_ctx* ctx, size_t w, const std::vector<CropCutDev>& cuts) {
    if (cuts.empty()) return SSW_OK;
    double bytes = 0.0;
    for (const CropCutDev& c : cuts) bytes += 2.0 * (double)c.cw3 * c.ch;
    StageTimer t(ctx, SSW_STAGE_CONVERT, ctx->stream, bytes);
    for (size_t i0 = 0; i0 < cuts.size(); i0 += CROP_BATCH) {
        const size_t m = std::min<size_t>(CROP_BATCH, cuts.size() - i0);
        CropCutBatch b{};
        unsigned cw3 = 0, ch = 0;
        for (size_t i = 0; i < m; ++i) { b.it[i] = cuts[i0 + i]; cw3 = std::max(cw3, b.it[i].cw3); ch = std::max(ch, b.it[i].ch); }
        const unsigned chunks = cw3 / 16 + 2;                               // an unaligned row touches one chunk more
        crop_cut_kernel<<<dim3((chunks + 255) / 256, ch, (unsigned)m), 256, 0, ctx->stream>>>((unsigned)(w * 3), b);
        SSW_HIP_CHECK(hipGetLastError());
    }
    return SSW_OK;
}

int complement_enqueue(ssw_ctx* ctx, const uint8_t* dev_base, size_t w, size_t h, const std::vector<CropCompDev>& comps) {
    if (comps.empty()) return SSW_OK;
    StageTimer t(ctx, SSW_STAGE_RESIZE, ctx->stream, (double)comps.size() * 6.0 * (double)w * h);
    const unsigned chunks = (unsigned)(w * 3 / 16 + 2);
    for (size_t i0 = 0; i0 < comps.size(); i0 += CROP_BATCH) {
        const size_t m = std::min<size_t>(CROP_BATCH, comps.size() - i0);
        CropCompBatch b{};
        std::copy(comps.begin() + i0, comps.begin() + i0 + m, b.it);
        crop_complement_kernel<<<dim3((chunks + 255) / 256, (unsigned)h, (unsigned)m), 256, 0, ctx->stream>>>(dev_base, (unsigned)(w * 3), (unsigned)h, b);
        SSW_HIP_CHECK(hipGetLastError());
    }
    return SSW_OK;
}

// ssw_restore_rgb8 for results that do not lie one behind the other
int restore_each(ssw_ctx* ctx, const uint8_t* dev_base, size_t w, size_t h, std::vector<RestoreJob>& jobs) {
    std::vector<RestoreJob> run;
    for (const RestoreJob& j : jobs) {
        if (restore_untouched(j.p, w, h)) {
            SSW_HIP_CHECK(hipMemcpyAsync(j.out, j.src, w * h * 3, hipMemcpyDeviceToDevice, ctx->stream));
            untimed_work(ctx);
        } else {
            run.push_back(j);
        }
    }
    return restore_enqueue(ctx, dev_base, w, h, run.data(), run.size());
}

// Both entry points.  searches == null: the placed form.
int crop_impl(ssw_ctx* ctx, const uint8_t* dev_base, const uint8_t* dev_frames, size_t n_frames, size_t w, size_t h, const ssw_crop_job* jobs,
              const ssw_crop_search* searches, size_t n_jobs, uint8_t* dev_out, uint8_t* dev_thumbs, ssw_placement* host_found, uint64_t* host_sad) {
    size_t thumbs_total = 0;
    SSW_TRY(crop_check(ctx, dev_base, dev_frames, n_frames, w, h, jobs, n_jobs, dev_out, dev_thumbs, &thumbs_total));
    const bool search = searches != nullptr;
    const size_t fb = w * h * 3;
    CtxGuard g(ctx);
    // the placed form knows every placement now: its tap tables go up before anything is enqueued
    if (!search) {
        std::vector<ssw_placement> pl;
        for (size_t i = 0; i < n_jobs; ++i)
            if (scaled(jobs[i])) pl.push_back(ssw_placement{jobs[i].tw, jobs[i].th, 3, jobs[i].x, jobs[i].y, jobs[i].cw, jobs[i].ch});
        SSW_TRY(restore_prepare(ctx, pl));
    }
    // what a job keeps in the workspace: its piece when a resize reads it, its thumbnail when the caller takes none
    auto need = [&](const ssw_crop_job& j) {
        const bool piece = scaled(j), thumb = !dev_thumbs && (scaled(j) || search);
        return (piece ? piece_bytes(j) : 0) + (thumb ? thumb_bytes(j) : 0);
    };
    std::vector<size_t> thumb_off(n_jobs + 1, 0);
    for (size_t i = 0; i < n_jobs; ++i) thumb_off[i + 1] = thumb_off[i] + thumb_bytes(jobs[i]);
    size_t ws_bytes = 0;
    for (size_t g0 = 0; g0 < n_jobs;) {
        size_t g1 = g0, bytes = 0;
        while (g1 < n_jobs && (g1 == g0 || bytes + need(jobs[g1]) <= CROP_GROUP_BYTES)) bytes += need(jobs[g1++]);
        ws_bytes = std::max(ws_bytes, bytes);
        g0 = g1;
    }
    if (ws_bytes) SSW_TRY(grow(ctx->shared.crop, ws_bytes));
    uint8_t* ws = ctx->shared.crop.as<uint8_t>();

    for (size_t g0 = 0; g0 < n_jobs;) {
        size_t g1 = g0, bytes = 0;
        while (g1 < n_jobs && (g1 == g0 || bytes + need(jobs[g1]) <= CROP_GROUP_BYTES)) bytes += need(jobs[g1++]);
        // workspace of the group: the pieces one behind the other, then the thumbnails; with dev_thumbs the thumbnails lie there
        std::vector<uint8_t*> piece(g1 - g0, nullptr), thumb(g1 - g0, nullptr);
        size_t at = 0;
        for (size_t i = g0; i < g1; ++i)
            if (scaled(jobs[i])) { piece[i - g0] = ws + at; at += piece_bytes(jobs[i]); }
        for (size_t i = g0; i < g1; ++i) {
            if (dev_thumbs) thumb[i - g0] = dev_thumbs + thumb_off[i];
            else if (scaled(jobs[i]) || search) { thumb[i - g0] = ws + at; at += thumb_bytes(jobs[i]); }
        }
        // 1. the cuts, and the placed, unscaled jobs whole
        std::vector<CropCutDev> cuts;
        std::vector<CropCompDev> comps;
        for (size_t i = g0; i < g1; ++i) {
            const ssw_crop_job& j = jobs[i];
            const uint8_t* frame = dev_frames + (size_t)j.frame * fb;
            uint8_t* dst = scaled(j) ? piece[i - g0] : thumb[i - g0];
            if (dst) cuts.push_back(CropCutDev{frame + ((size_t)j.y * w + j.x) * 3, dst, j.cw * 3, j.ch});
            if (!scaled(j) && !search) comps.push_back(CropCompDev{frame, dev_out + i * fb, j.x * 3, j.cw * 3, j.y, j.ch});
        }
        SSW_TRY(cut_enqueue(ctx, w, cuts));
        SSW_TRY(complement_enqueue(ctx, dev_base, w, h, comps));
        // 2. the thumbnails: consecutive jobs of one class are one ssw_resample_rgb8 call (their pieces and thumbnails are neighbours)
        for (size_t i0 = g0; i0 < g1;) {
            size_t i1 = i0 + 1;
            if (!scaled(jobs[i0])) { i0 = i1; continue; }
            while (i1 < g1 && scaled(jobs[i1]) && same_class(jobs[i0], jobs[i1])) ++i1;
            const ssw_crop_job& j = jobs[i0];
            SSW_TRY(ssw_resample_rgb8(ctx, piece[i0 - g0], i1 - i0, j.cw, j.ch, j.tw, j.th, (int)j.filter, thumb[i0 - g0]));
            i0 = i1;
        }
        // 3. the placements: given, or what the searches answer (these wait for the stream)
        std::vector<RestoreJob> back;
        if (!search) {
            for (size_t i = g0; i < g1; ++i) {
                const ssw_crop_job& j = jobs[i];
                if (scaled(j)) back.push_back(RestoreJob{thumb[i - g0], dev_out + i * fb, ssw_placement{j.tw, j.th, 3, j.x, j.y, j.cw, j.ch}});
            }
        } else {
            for (int ranged = 0; ranged < 2; ++ranged) {
                std::vector<size_t> which;
                std::vector<const void*> ptrs;
                std::vector<ssw_placement> pl;
                std::vector<ssw_scale_range> rg;
                for (size_t i = g0; i < g1; ++i) {
                    const bool r = searches[i].wmin != 0 || searches[i].wmax != 0;
                    if ((int)r != ranged) continue;
                    const ssw_crop_job& j = jobs[i];
                    which.push_back(i);
                    ptrs.push_back(thumb[i - g0]);
                    pl.push_back(ssw_placement{scaled(j) ? j.tw : j.cw, scaled(j) ? j.th : j.ch, 3, 0, 0, 0, 0});
                    rg.push_back(ssw_scale_range{searches[i].wmin, searches[i].wmax});
                }
                if (which.empty()) continue;
                std::vector<uint64_t> sad(which.size());
                if (ranged) SSW_TRY(ssw_locate_scaled_rgb8(ctx, dev_base, w, h, ptrs.data(), pl.data(), rg.data(), which.size(), sad.data()));
                else        SSW_TRY(ssw_locate_rgb8(ctx, dev_base, w, h, ptrs.data(), pl.data(), which.size(), sad.data()));
                for (size_t q = 0; q < which.size(); ++q) {
                    if (!ranged) { pl[q].pw = pl[q].w; pl[q].ph = pl[q].h; }
                    host_found[which[q]] = pl[q];
                    host_sad[which[q]] = sad[q];
                    back.push_back(RestoreJob{(const uint8_t*)ptrs[q], dev_out + which[q] * fb, pl[q]});
                }
            }
            std::vector<ssw_placement> pl;
            for (const RestoreJob& r : back) pl.push_back(r.p);
            SSW_TRY(restore_prepare(ctx, pl));
        }
        SSW_TRY(restore_each(ctx, dev_base, w, h, back));
        g0 = g1;
    }
    return SSW_OK;
}

}  // namespace
}  // namespace host
}  // namespace ssw

extern "C" int ssw_crop_attack_rgb8(ssw_ctx* ctx, const uint8_t* dev_base, const uint8_t* dev_frames, size_t n_frames, size_t w, size_t h,
                                    const ssw_crop_job* jobs, size_t n_jobs, uint8_t* dev_out, uint8_t* dev_thumbs) {
    if (!ctx) return SSW_ERR_BAD_ARG;
    if (n_jobs == 0) return SSW_OK;
    return ssw::host::crop_impl(ctx, dev_base, dev_frames, n_frames, w, h, jobs, nullptr, n_jobs, dev_out, dev_thumbs, nullptr, nullptr);
}

extern "C" int ssw_crop_search_attack_rgb8(ssw_ctx* ctx, const uint8_t* dev_base, const uint8_t* dev_frames, size_t n_frames, size_t w, size_t h,
                                           const ssw_crop_job* jobs, const ssw_crop_search* searches, size_t n_jobs, uint8_t* dev_out,
                                           uint8_t* dev_thumbs, ssw_placement* host_found, uint64_t* host_sad) {
    if (!ctx) return SSW_ERR_BAD_ARG;
    if (n_jobs == 0) return SSW_OK;
    if (!searches || !host_found || !host_sad) return SSW_ERR_BAD_ARG;
    return ssw::host::crop_impl(ctx, dev_base, dev_frames, n_frames, w, h, jobs, searches, n_jobs, dev_out, dev_thumbs, host_found, host_sad);
}
