// Locating cut-outs of a turned copy (ssw_locate_turned_rgb8): a search over the angle of a rotation AND the position of a crop.
// For every rung of a ladder of angles 0.25 degrees apart the suspect's luma is turned back about its own centre into a template
// (integer bilinear taps, as large as the turned-back suspect holds), the template's 8 x 8 box means are searched for over the
// original's box planes, the 4 best rungs are refined -- every angle within 7 / 32 degrees of them, full-resolution templates,
// windowed searches of ssw_locate_rgb8 -- and the best of those is the answer.  include/ssw.h states the definition; every
// quantity is an integer, so the result equals the numpy restatement of tests/test_locate_turned_cpu.py exactly.  The reference
// has no counterpart.
//
// Kernel (the planes and the searches are locate.hip's):
//   turned_template_kernel   THE HOT PATH THAT IS NEW, both epilogues: a block takes a tile of 32 x 32 template pixels of one
//                            (suspect, angle) and the staged box of the suspect's luma plane: turned_tile.hpp, with f = 1 and
//                            -S.  A lane makes 4 pixels of a row, one word.  The ladder's epilogue puts the words into LDS and
//                            stores only the tile's 8 x 8 box means T_j (tiles are multiples of 8 pixels: no box straddles two
//                            blocks), so a rung's template never reaches HBM at full resolution; the refinement's epilogue
//                            stores the word.
// Launch descriptors travel as kernel arguments, 32 (suspect, angle) items per launch, like locate.hip's.
#include <algorithm>
#include <cstring>
#include <vector>

#include "ssw_host.hpp"
#include "turned_tables.hpp"
#include "turned_tile.hpp"

namespace ssw {

struct TurnedDev {
    const uint8_t* ls;           // the suspect's luma plane [sh][lpitch]
    uint8_t* out;                // boxes: T_j [th / 8][opitch]; else the template [th][opitch], opitch % 4 == 0
    uint32_t lpitch, sw, sh, tw, th, opitch, tiles_x, tile_begin, boxes;
    int32_t C, S;
};
struct TurnedBatch { TurnedDev it[host::LOCATE_BATCH]; };

// grid: (tiles of all items of the launch); block: TURN_THREADS.  A lane: 4 pixels of one row of the tile
__global__ __launch_bounds__(TURN_THREADS) void turned_template_kernel(TurnedBatch b, unsigned n) {
    __shared__ TurnedBox s_box;
    __shared__ uint32_t s_t[TURN_TILE_H][TURN_TILE_W / 4];
    unsigned s = 0;
    while (s + 1 < n && blockIdx.x >= b.it[s + 1].tile_begin) ++s;
    const TurnedDev& d = b.it[s];
    const unsigned t = threadIdx.x, tile = blockIdx.x - d.tile_begin;
    const Turn m{d.C, -d.S, 1, 17, d.sw, d.sh, d.tw, d.th};            // the suspect's plane turned BACK into the template
    const uint32_t Xt = (tile % d.tiles_x) * TURN_TILE_W, Yt = (tile / d.tiles_x) * TURN_TILE_H;
    const int nx = (int)min(TURN_TILE_W, d.tw - Xt), ny = (int)min(TURN_TILE_H, d.th - Yt);          // multiples of 8
    const TurnedTile tl = turned_tile(m, Xt, Yt, nx, ny);
    turned_stage(s_box, d.ls, d.lpitch, d.sw, d.sh, tl);               // (every tap of a template is inside the plane)
    const int dx0 = 4 * (int)(t % (TURN_TILE_W / 4)), dy = (int)(t / (TURN_TILE_W / 4));
    const bool mine = dx0 < nx && dy < ny;
    uint32_t word = 0;
    if (mine) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            int32_t lrx, lry;
            turned_pixel(m, tl, dx0 + k, dy, &lrx, &lry);
            const int32_t X0 = min(max(lrx >> m.shift, 0), tl.bw - 2), Y0 = min(max(lry >> m.shift, 0), tl.bh - 2);       // (inside the box as it is)
            word |= turned_value(s_box, m, X0, Y0, lrx, lry) << (8 * k);
        }
    }
    if (!d.boxes) {                                                              // (uniform)
        if (mine) *reinterpret_cast<uint32_t*>(d.out + (size_t)(Yt + dy) * d.opitch + Xt + dx0) = word;
        return;
    }
    s_t[dy][dx0 / 4] = word;
    __syncthreads();
    // the boxes of the tile: one thread each, 16 words
    const unsigned nbx = (unsigned)nx / 8, nby = (unsigned)ny / 8;
    if (t < nbx * nby) {
        const unsigned bk = t / nbx, bi = t - bk * nbx;
        uint32_t sum = 32;
#pragma unroll
        for (unsigned j = 0; j < 8; ++j) {
            sum = __builtin_amdgcn_sad_u8(s_t[8 * bk + j][2 * bi], 0u, sum);
            sum = __builtin_amdgcn_sad_u8(s_t[8 * bk + j][2 * bi + 1], 0u, sum);
        }
        d.out[(size_t)(Yt / 8 + bk) * d.opitch + Xt / 8 + bi] = (uint8_t)(sum >> 6);
    }
}

namespace host {
namespace {

constexpr size_t TRN_GROUP_BYTES = (size_t)256 << 20;        // workspace of one group: suspects' planes, a launch's boxes and D, templates

struct TurnedSuspect { const uint8_t* ls; uint32_t sw, sh, lpitch; };
// one (suspect, angle): the template and where it goes
struct TurnedItem { uint32_t sus; int32_t n; uint32_t tw, th, opitch; size_t bytes; uint8_t* out; };

TurnedItem turned_item(uint32_t sus, int32_t n, uint32_t tw, uint32_t th, bool boxes) {
    TurnedItem it{sus, n, tw, th, 0, 0, nullptr};
    it.opitch = (uint32_t)round_up(boxes ? tw / 8 : tw, 4);
    it.bytes = round_up((size_t)it.opitch * (boxes ? th / 8 : th), 256);
    return it;
}

// the template launches of items [b0, b1), at most LOCATE_BATCH a launch; timed as a resize (bytes: the suspect's plane in, the template out)
int enqueue_templates(ssw_ctx* ctx, const std::vector<TurnedSuspect>& sus, const std::vector<TurnedItem>& items, size_t b0, size_t b1, bool boxes) {
    double bytes = 0.0;
    for (size_t i = b0; i < b1; ++i) bytes += (double)items[i].tw * items[i].th + (double)items[i].opitch * (boxes ? items[i].th / 8 : items[i].th);
    StageTimer t(ctx, SSW_STAGE_RESIZE, ctx->stream, bytes);
    for (size_t l0 = b0; l0 < b1; l0 += LOCATE_BATCH) {
        const unsigned m = (unsigned)std::min<size_t>(LOCATE_BATCH, b1 - l0);
        TurnedBatch tb{};
        unsigned tiles = 0;
        for (unsigned s = 0; s < m; ++s) {
            const TurnedItem& it = items[l0 + s];
            const TurnedSuspect& su = sus[it.sus];
            TurnedDev& d = tb.it[s];
            d.ls = su.ls; d.out = it.out; d.lpitch = su.lpitch; d.sw = su.sw; d.sh = su.sh; d.tw = it.tw; d.th = it.th; d.opitch = it.opitch;
            d.tiles_x = (it.tw + TURN_TILE_W - 1) / TURN_TILE_W; d.tile_begin = tiles; d.boxes = boxes ? 1u : 0u;
            angle_table(it.n, &d.C, &d.S);
            tiles += d.tiles_x * ((it.th + TURN_TILE_H - 1) / TURN_TILE_H);
        }
        turned_template_kernel<<<tiles, TURN_THREADS, 0, ctx->stream>>>(tb, m);
        SSW_HIP_CHECK(hipGetLastError());
    }
    return SSW_OK;
}

// the luma planes of the suspects [i0, i1) into locate.turned_luma
int suspect_planes(ssw_ctx* ctx, const void* const* dev_suspects, const ssw_turned_shape* shapes, size_t i0, size_t i1, std::vector<TurnedSuspect>* sus) {
    size_t total = 0;
    std::vector<size_t> off;
    for (size_t i = i0; i < i1; ++i) {
        off.push_back(total);
        total += round_up(round_up(shapes[i].w, 4) * (size_t)shapes[i].h, 256);
    }
    uint8_t* planes = nullptr;
    SSW_TRY(grow_as(ctx->locate.turned_luma, total + 16, planes));
    StageTimer t(ctx, SSW_STAGE_LOCATE, ctx->stream, 4.0 * (double)total);
    sus->clear();
    for (size_t i = i0; i < i1; ++i) {
        const TurnedSuspect s{planes + off[i - i0], shapes[i].w, shapes[i].h, (uint32_t)round_up(shapes[i].w, 4)};
        SSW_TRY(locate_luma_planes(ctx, (const uint8_t*)dev_suspects[i], 1, s.sw, s.sh, planes + off[i - i0], 0, s.lpitch));
        sus->push_back(s);
    }
    return SSW_OK;
}

struct RungEntry { bool live; uint32_t tw, th, nx, x, y; uint64_t D; };

// The suspects [i0, i1) of a call: one group (their planes fit the workspace).  Waits for the stream twice -- for the ladder's
// per-rung minima (the kept rungs decide which templates are made next, and their sizes shape the launches), and for the answer
// -- and once more for every further 256 MiB of the refinement's templates.
int turned_group(ssw_ctx* ctx, const uint8_t* dev_base, size_t w, size_t h, const void* const* dev_suspects, const ssw_turned_shape* shapes,
                 size_t i0, size_t i1, int j0, int j1, ssw_turned_found* found, uint64_t* host_rungs) {
    hipStream_t st = ctx->stream;
    const size_t n_rungs = (size_t)(j1 - j0 + 1);
    // the ladder's rungs; a dropped one has no item
    std::vector<TurnedItem> items;
    std::vector<std::vector<RungEntry>> entry(i1 - i0, std::vector<RungEntry>(n_rungs, RungEntry{}));
    std::vector<size_t> item_rung;
    for (size_t i = i0; i < i1; ++i) {
        bool any = false;
        for (int j = j0; j <= j1; ++j) {
            uint32_t tw = 0, th = 0;
            if (!turned_usable_size(w, h, shapes[i].w, shapes[i].h, ANGLE_RUNG_STEP * j, &tw, &th)) continue;
            RungEntry& e = entry[i - i0][(size_t)(j - j0)];
            e.live = true; e.tw = tw; e.th = th; e.nx = (uint32_t)((w - tw) / TURNED_STRIDE + 1);
            if ((uint64_t)e.nx * ((h - th) / TURNED_STRIDE + 1) > 0xFFFFFFFFull) return SSW_ERR_UNSUPPORTED;
            items.push_back(turned_item((uint32_t)(i - i0), ANGLE_RUNG_STEP * j, tw, th, true));
            item_rung.push_back((size_t)(j - j0));
            any = true;
        }
        if (!any) return SSW_ERR_BAD_DIMS;
    }
    std::vector<TurnedSuspect> sus;
    SSW_TRY(suspect_planes(ctx, dev_suspects, shapes, i0, i1, &sus));
    const uint8_t* planes = nullptr;
    unsigned qpitch = 0, qrows = 0;
    size_t plane_stride = 0;
    SSW_TRY(locate_box8_planes(ctx, dev_base, w, h, &planes, &qpitch, &qrows, &plane_stride));
    const size_t nr = items.size();
    uint64_t* keys = nullptr;
    SSW_TRY(grow_as(ctx->locate.keys, nr * LOCATE_KEY_STRIDE * sizeof(uint64_t), keys));
    SSW_HIP_CHECK(hipMemsetAsync(keys, 0xFF, nr * LOCATE_KEY_STRIDE * sizeof(uint64_t), st));
    untimed_work(ctx);
    // launches of at most LOCATE_BATCH rungs and a group's bytes of workspace (T and D of each)
    auto d_bytes = [&](const TurnedItem& it) { return round_up((size_t)((w - it.tw) / TURNED_STRIDE + 1) * ((h - it.th) / TURNED_STRIDE + 1) * 4, 256); };
    for (size_t b0 = 0; b0 < nr;) {
        size_t b1 = b0, bytes = 0;
        while (b1 < nr && b1 - b0 < LOCATE_BATCH && (b1 == b0 || bytes + items[b1].bytes + d_bytes(items[b1]) <= TRN_GROUP_BYTES)) {
            bytes += items[b1].bytes + d_bytes(items[b1]);
            ++b1;
        }
        uint8_t* ws = nullptr;
        SSW_TRY(grow_as(ctx->locate.group, bytes + 16, ws));
        BoxSearch bs[LOCATE_BATCH];
        size_t o = 0;
        for (size_t i = b0; i < b1; ++i) {
            TurnedItem& it = items[i];
            it.out = ws + o;
            bs[i - b0] = BoxSearch{it.out, (uint32_t*)(ws + o + it.bytes), it.opitch, it.tw / TURNED_BOX, it.th / TURNED_BOX,
                                   (uint32_t)((w - it.tw) / TURNED_STRIDE + 1), (uint32_t)((h - it.th) / TURNED_STRIDE + 1)};
            o += it.bytes + d_bytes(it);
        }
        SSW_TRY(enqueue_templates(ctx, sus, items, b0, b1, true));
        SSW_TRY(locate_box_searches(ctx, planes, qpitch, qrows, plane_stride, bs, (unsigned)(b1 - b0), keys + b0 * LOCATE_KEY_STRIDE));
        b0 = b1;
    }
    std::vector<uint64_t> hk(nr * LOCATE_KEY_STRIDE);
    SSW_HIP_CHECK(hipMemcpyAsync(hk.data(), keys, hk.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    untimed_work(ctx);
    SSW_HIP_CHECK(hipStreamSynchronize(st));
    for (size_t r = 0; r < nr; ++r) {
        RungEntry& e = entry[items[r].sus][item_rung[r]];
        const uint32_t idx = (uint32_t)hk[r * LOCATE_KEY_STRIDE];
        e.D = hk[r * LOCATE_KEY_STRIDE] >> 32;
        e.x = TURNED_STRIDE * (idx % e.nx); e.y = TURNED_STRIDE * (idx / e.nx);
    }
    // on the host: the 4 rungs with the smallest D / n_j, then the windowed searches of every angle near them
    std::vector<TurnedItem> jobs;
    std::vector<LocWindow> win;
    for (size_t i = i0; i < i1; ++i) {
        const std::vector<RungEntry>& en = entry[i - i0];
        std::vector<size_t> order;
        for (size_t r = 0; r < n_rungs; ++r) {
            const RungEntry& e = en[r];
            if (host_rungs) {
                uint64_t* o = host_rungs + (i * n_rungs + r) * 4;
                o[0] = e.live ? e.D : 0; o[1] = e.live ? (uint64_t)(e.tw / TURNED_BOX) * (e.th / TURNED_BOX) : 0; o[2] = e.live ? e.x : 0; o[3] = e.live ? e.y : 0;
            }
            if (e.live) order.push_back(r);
        }
        auto N = [&](size_t r) { return (uint64_t)(en[r].tw / TURNED_BOX) * (en[r].th / TURNED_BOX); };       // D n < 2^32 2^26
        std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return en[a].D * N(b) < en[b].D * N(a); });
        if (order.size() > ANGLE_KEEP) order.resize(ANGLE_KEEP);
        std::vector<int32_t> seen;
        for (size_t r : order) {
            const RungEntry& e = en[r];
            const int32_t mid = ANGLE_RUNG_STEP * (j0 + (int32_t)r);
            for (int32_t a = mid - ANGLE_NEAR; a <= mid + ANGLE_NEAR; ++a) {
                if (a < ANGLE_RUNG_STEP * j0 || a > ANGLE_RUNG_STEP * j1 || std::find(seen.begin(), seen.end(), a) != seen.end()) continue;
                seen.push_back(a);
                uint32_t tw = 0, th = 0;
                if (!turned_usable_size(w, h, shapes[i].w, shapes[i].h, a, &tw, &th)) continue;
                const int64_t cx = (2 * (int64_t)e.x + e.tw - tw) >> 1, cy = (2 * (int64_t)e.y + e.th - th) >> 1;
                const int64_t x0 = std::max<int64_t>(0, cx - TURNED_NEAR_XY), x1 = std::min<int64_t>((int64_t)w - tw, cx + TURNED_NEAR_XY);
                const int64_t y0 = std::max<int64_t>(0, cy - TURNED_NEAR_XY), y1 = std::min<int64_t>((int64_t)h - th, cy + TURNED_NEAR_XY);
                if (x0 > x1 || y0 > y1) continue;
                jobs.push_back(turned_item((uint32_t)(i - i0), a, tw, th, false));
                win.push_back(LocWindow{(uint32_t)x0, (uint32_t)x1, (uint32_t)y0, (uint32_t)y1, false});
            }
        }
    }
    // the refinement: the templates of as many searches as the workspace holds, then ssw_locate_rgb8's search of each in its window
    std::vector<char> have(i1 - i0, 0);
    for (size_t b0 = 0; b0 < jobs.size();) {
        size_t b1 = b0, bytes = 0;
        while (b1 < jobs.size() && (b1 == b0 || bytes + jobs[b1].bytes <= TRN_GROUP_BYTES)) bytes += jobs[b1++].bytes;
        uint8_t* ws = nullptr;
        SSW_TRY(grow_as(ctx->locate.turned_templates, bytes + 16, ws));
        std::vector<const void*> ptr;
        std::vector<ssw_placement> pl;
        size_t o = 0;
        for (size_t q = b0; q < b1; ++q) {
            jobs[q].out = ws + o;
            o += jobs[q].bytes;
            ptr.push_back(jobs[q].out);
            pl.push_back(ssw_placement{jobs[q].tw, jobs[q].th, 3u, 0u, 0u, jobs[q].tw, jobs[q].th});
        }
        SSW_TRY(enqueue_templates(ctx, sus, jobs, b0, b1, false));
        std::vector<uint64_t> res(2 * (b1 - b0));
        const std::vector<LocWindow> wn(win.begin() + (ptrdiff_t)b0, win.begin() + (ptrdiff_t)b1);
        SSW_TRY(locate_impl(ctx, dev_base, w, h, ptr.data(), pl, res.data(), &wn, true));
        for (size_t q = b0; q < b1; ++q) {
            const TurnedItem& jb = jobs[q];
            ssw_turned_found a{jb.n, (uint32_t)res[2 * (q - b0) + 1], (uint32_t)(res[2 * (q - b0) + 1] >> 32), jb.tw, jb.th, (uint32_t)n_rungs, res[2 * (q - b0)]};
            ssw_turned_found& b = found[i0 + jb.sus];
            bool better = !have[jb.sus];
            if (!better) {                                              // smallest SAD / (tw th), then n, y, x; 255 * 2^32 * 2^32 does not fit: 128 bits
                const unsigned __int128 l = (unsigned __int128)a.sad * ((uint64_t)b.tw * b.th), r = (unsigned __int128)b.sad * ((uint64_t)a.tw * a.th);
                better = l != r ? l < r : a.n != b.n ? a.n < b.n : a.y != b.y ? a.y < b.y : a.x < b.x;
            }
            if (better) { b = a; have[jb.sus] = 1; }
        }
        b0 = b1;
    }
    return SSW_OK;
}

}  // namespace
}  // namespace host
}  // namespace ssw

extern "C" int ssw_locate_turned_rgb8(ssw_ctx* ctx, const uint8_t* dev_base, size_t w, size_t h, const void* const* dev_suspects,
                                      const ssw_turned_shape* shapes, size_t n, double amin, double amax, ssw_turned_found* host_found,
                                      uint64_t* host_rungs) {
    using namespace ssw;
    using namespace ssw::host;
    if (!ctx) return SSW_ERR_BAD_ARG;
    if (n == 0) return SSW_OK;
    int j0 = 0, j1 = 0;
    if (!dev_base || !dev_suspects || !shapes || !host_found || !angle_rungs(amin, amax, &j0, &j1)) return SSW_ERR_BAD_ARG;
    for (size_t i = 0; i < n; ++i)
        if (!dev_suspects[i] || (shapes[i].channels != 3 && shapes[i].channels != 4)) return SSW_ERR_BAD_ARG;
    if (w == 0 || h == 0 || w > 65535 || h > 65535) return SSW_ERR_BAD_DIMS;
    for (size_t i = 0; i < n; ++i)
        if (shapes[i].w == 0 || shapes[i].h == 0 || shapes[i].w > 65535 || shapes[i].h > 65535) return SSW_ERR_BAD_DIMS;
    if (w < TURNED_SIDE_MIN || h < TURNED_SIDE_MIN) return SSW_ERR_BAD_DIMS;          // no template fits: every rung is dropped
    for (size_t i = 0; i < n; ++i)
        if (shapes[i].channels == 4) return SSW_ERR_UNSUPPORTED;
    CtxGuard g(ctx);
    // groups of suspects whose luma planes fit the workspace (one suspect's, if larger)
    for (size_t i0 = 0; i0 < n;) {
        size_t i1 = i0, bytes = 0;
        while (i1 < n && (i1 == i0 || bytes + (size_t)shapes[i1].w * shapes[i1].h <= TRN_GROUP_BYTES)) {
            bytes += (size_t)shapes[i1].w * shapes[i1].h;
            ++i1;
        }
        SSW_TRY(turned_group(ctx, dev_base, w, h, dev_suspects, shapes, i0, i1, j0, j1, host_found, host_rungs));
        i0 = i1;
    }
    return SSW_OK;
}

extern "C" int ssw_locate_turned_rung_boxes(ssw_ctx* ctx, const void* dev_suspect, size_t sw, size_t sh, int32_t n, uint32_t* tw, uint32_t* th,
                                            uint8_t* host_boxes) {
    using namespace ssw;
    using namespace ssw::host;
    if (!ctx || !dev_suspect || !tw || !th || n < -ANGLE_PER_DEGREE * 45 || n > ANGLE_PER_DEGREE * 45) return SSW_ERR_BAD_ARG;
    if (sw == 0 || sh == 0 || sw > 65535 || sh > 65535) return SSW_ERR_BAD_DIMS;
    if (!turned_template_size((uint32_t)sw, (uint32_t)sh, n, tw, th)) return SSW_ERR_BAD_DIMS;
    if (!host_boxes) return SSW_OK;                                     // the size alone
    CtxGuard g(ctx);
    const ssw_turned_shape shape{(uint32_t)sw, (uint32_t)sh, 3u};
    std::vector<TurnedSuspect> sus;
    SSW_TRY(suspect_planes(ctx, &dev_suspect, &shape, 0, 1, &sus));
    std::vector<TurnedItem> items{turned_item(0u, n, *tw, *th, true)};
    SSW_TRY(grow_as(ctx->locate.group, items[0].bytes + 16, items[0].out));
    SSW_TRY(enqueue_templates(ctx, sus, items, 0, 1, true));
    std::vector<uint8_t> t((size_t)items[0].opitch * (*th / 8));
    SSW_HIP_CHECK(hipMemcpyAsync(t.data(), items[0].out, t.size(), hipMemcpyDeviceToHost, ctx->stream));
    untimed_work(ctx);
    SSW_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    for (uint32_t k = 0; k < *th / 8; ++k) std::memcpy(host_boxes + (size_t)k * (*tw / 8), t.data() + (size_t)k * items[0].opitch, *tw / 8);
    return SSW_OK;
}
