// Orchestration of the reference's call stacks on the device: the 2-D transform as a chain of stages
// (operand pre-passes = HBM-bound, basis GEMMs = MFMA-bound), the pruned transform of derived frames, and
// the two-lane pipelines behind ssw_batch_embed / ssw_batch_extract.
//
// Two lanes, two streams.  A chunk's stages depend on each other in sequence, and they alternate between
// HBM-bound and MFMA-bound kernels; a single stream therefore leaves the matrix cores idle during ~13 % of
// a 4K step (25 % at full HD) and HBM idle for the rest.  The batch pipelines keep two chunks in flight,
// each with its own workspace ("lane"): every GEMM stage goes to the context's stream, every HBM-bound
// stage to `aux_stream`, stages are enqueued round-robin over the lanes, and a lane crosses from one
// stream to the other through an event.  GEMM launches never overlap each other (one stream), so their
// event timings stay meaningful; what overlaps is one lane's pre-pass / selection / colour conversion with
// the other lane's GEMMs.  Results are bit-identical to the serial order (same kernels, same chunks).
#include <algorithm>
#include <cmath>
#include <cstring>

#include "ssw_host.hpp"
#include "dct_pair_split.hpp"

#include <array>
#include <cstdlib>

namespace ssw {
namespace host {

// ---- small helpers ------------------------------------------------------------------------------------
namespace { thread_local ssw_ctx* tl_ctx = nullptr; }
CtxGuard::CtxGuard(ssw_ctx* ctx) : dg(ctx->device), prev(tl_ctx) {
    tl_ctx = ctx;
    if (prev != ctx) { ctx->tail_event = nullptr; ctx->tail_fresh = false; }     // timer events are shared inside one call only
    // buffers retired by grow() during the previous call: nothing built then is still to be enqueued (hipFree waits for
    // work in flight); nested guards (prev == ctx) leave them to the outermost one
    if (prev != ctx && !ctx->retired.empty()) {
        for (void* p : ctx->retired) (void)hipFree(p);
        ctx->retired.clear();
    }
}
CtxGuard::~CtxGuard() { tl_ctx = prev; }

size_t plane_pool_flush(ssw_ctx* ctx) {
    size_t bytes = ctx->plane_pool_bytes;
    for (auto& kv : ctx->plane_pool) (void)hipFree(kv.second);
    ctx->plane_pool.clear();
    ctx->plane_pool_bytes = 0;
    for (auto& sp : ctx->rgb_spares) { (void)hipFree(sp.p); (void)hipEventDestroy(sp.released); bytes += sp.bytes; }
    ctx->rgb_spares.clear();
    return bytes;
}

// The device ring of the host-image streaming entry points (ssw_stream.hip: 3 slots x two buffers of a group of frames,
// ~1.2 GB at the default group size) stays allocated between calls; under memory pressure it goes back like the plane pool.
size_t host_stream_release(ssw_ctx* ctx) {
    ssw_ctx::HostStream& hs = ctx->hs;
    if (hs.active) return 0;
    size_t bytes = 0;
    for (int s = 0; s < ssw_ctx::HostStream::NB; ++s)
        for (ssw_ctx::Buf* b : {&hs.in[s], &hs.in2[s], &hs.out[s]})
            if (b->p) { bytes += b->bytes; (void)hipFree(b->p); b->p = nullptr; b->bytes = 0; }
    return bytes;
}

int dev_malloc(void** p, size_t bytes) {
    *p = nullptr;
    hipError_t e = hipMalloc(p, bytes ? bytes : 16);
    if (e == hipSuccess) return SSW_OK;
    (void)hipGetLastError();
    if (tl_ctx && (!tl_ctx->plane_pool.empty() || !tl_ctx->rgb_spares.empty())) {      // spare planes of destroyed handles: give them back first
        (void)plane_pool_flush(tl_ctx);
        e = hipMalloc(p, bytes ? bytes : 16);
        if (e == hipSuccess) return SSW_OK;
        (void)hipGetLastError();
    }
    if (tl_ctx && host_stream_release(tl_ctx)) {                   // then the idle streaming ring
        e = hipMalloc(p, bytes ? bytes : 16);
        if (e == hipSuccess) return SSW_OK;
        (void)hipGetLastError();
    }
    *p = nullptr;
    set_last_error(std::string("hipMalloc(") + std::to_string(bytes) + " bytes): " + hipGetErrorString(e));
    return SSW_ERR_OUT_OF_MEMORY;
}

int grow(ssw_ctx::Buf& b, size_t bytes) {
    if (b.bytes >= bytes && b.p) return SSW_OK;
    // A buffer that grows in the middle of a call may already be captured by stages built earlier in the same chain (the
    // lane's slots have several roles: ssw_internal.hpp, Lane): the old allocation is retired, not freed -- those stages
    // keep working on it, the later ones use the new one -- and the next entry into the library frees it (CtxGuard).
    // Without a context in scope: free now (hipFree waits for work in flight).
    if (b.p) {
        if (tl_ctx) tl_ctx->retired.push_back(b.p);
        else SSW_HIP_CHECK(hipFree(b.p));
        b.p = nullptr; b.bytes = 0;
    }
    SSW_ALLOC(&b.p, bytes);
    b.bytes = bytes ? bytes : 16;
    return SSW_OK;
}

void release(ssw_ctx::Buf& b) {
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr;
    b.bytes = 0;
}

void release_select(SelectWorkspace& s) {
    if (s.hist) (void)hipFree(s.hist);
    if (s.ctrl) (void)hipFree(s.ctrl);
    if (s.cand) (void)hipFree(s.cand);
    s = SelectWorkspace();
}

int grow_select(hipStream_t st, SelectWorkspace& s, size_t frames, size_t k) {
    const size_t want = select_cand_capacity(k);
    if (s.frames >= frames && s.cap >= want && s.hist) return SSW_OK;
    const size_t nf = std::max(frames, s.frames), cap = std::max(want, s.cap);
    release_select(s);
    SSW_ALLOC(&s.hist, nf * 2048 * sizeof(uint32_t));
    SSW_ALLOC(&s.ctrl, nf * 4 * sizeof(uint32_t));
    SSW_ALLOC(&s.cand, nf * cap * sizeof(uint64_t));
    SSW_HIP_CHECK(hipMemsetAsync(s.hist, 0, nf * 2048 * sizeof(uint32_t), st));   // see select.hip:
    SSW_HIP_CHECK(hipMemsetAsync(s.ctrl, 0, nf * 4 * sizeof(uint32_t), st));      // zero between uses
    untimed_work(tl_ctx);
    s.frames = nf;
    s.cap = cap;
    return SSW_OK;
}

// Stage timers share their boundary events (r5): a stage that starts right after another one ended on the same stream --
// nothing enqueued in between: the stages of a chain, a "main launch" timer nested at the start or the end of its pass --
// takes the event that is already in the stream instead of recording a second one.  An event record is a barrier in the
// queue (~3 us during which the next kernel cannot overlap the previous one's tail): a single-frame embed had 28 of them in
// 0.6 ms of kernels.  ctx->tail_event is the last event recorded by a timer, valid while ctx->tail_fresh: cleared by the next
// timer's own launches, by untimed_work() (ssw_host.hpp) -- called wherever something is enqueued outside a timer: the lanes'
// hops / done records / stagger waits, the pruned transform's table launches, basis generation, workspace memsets, copies,
// the upload / download hand-offs of the handle and streaming entry points -- and at every entry into the library.
static hipEvent_t timer_event(ssw_ctx* ctx, hipStream_t st) {
    if (ctx->tail_event && ctx->tail_fresh && ctx->tail_stream == st) return ctx->tail_event;
    hipEvent_t e = nullptr;
    if (!ctx->free_events.empty()) { e = ctx->free_events.back(); ctx->free_events.pop_back(); }
    else if (hipEventCreateWithFlags(&e, hipEventReleaseToDevice) != hipSuccess) return nullptr;
    if (hipEventRecord(e, st) != hipSuccess) { ctx->free_events.push_back(e); return nullptr; }
    ctx->tail_event = e; ctx->tail_stream = st; ctx->tail_fresh = true;
    return e;
}
StageTimer::StageTimer(ssw_ctx* c, int s, hipStream_t stream, double work, int alias_stage) : ctx(c), stage(s), st(stream), alias(alias_stage) {
    if (!ctx->timing) return;
    ctx->stage_work[stage] += work;
    if (alias >= 0) ctx->stage_work[alias] += work;
    const bool gemm = stage == SSW_STAGE_DCT_ROW || stage == SSW_STAGE_DCT_COL || stage == SSW_STAGE_DCT_ROW_MAIN || stage == SSW_STAGE_DCT_COL_MAIN;
    if (!gemm) ctx->stage_bytes[stage] += work;
    a = timer_event(ctx, st);
    ctx->tail_fresh = false;                  // the stage's launches follow: its end needs an event of its own
    armed = a != nullptr;
}
void StageTimer::traffic(double bytes) {
    if (ctx->timing) ctx->stage_bytes[stage] += bytes;
}
StageTimer::~StageTimer() {
    if (!ctx->timing || !armed) return;
    // (a nested timer that just ended left a fresh event: the outer stage ends at the same point)
    b = timer_event(ctx, st);
    if (b) ctx->pending.push_back({stage, a, b, alias});
}

namespace { int base_prune_bill(ssw_ctx* ctx); }       // (beside the base reader's set-up, below)
int flush_timers(ssw_ctx* ctx) {
    std::vector<hipEvent_t> used;
    for (auto& p : ctx->pending) {
        float ms = 0.f;
        SSW_HIP_CHECK(hipEventSynchronize(p.b));
        SSW_HIP_CHECK(hipEventElapsedTime(&ms, p.a, p.b));
        ctx->stage_ms[p.stage] += ms;
        ctx->stage_launches[p.stage] += 1;
        if (p.alias >= 0) { ctx->stage_ms[p.alias] += ms; ctx->stage_launches[p.alias] += 1; }
        used.push_back(p.a);
        used.push_back(p.b);
    }
    ctx->pending.clear();
    // shared boundary events appear in two entries: each goes back to the pool once
    std::sort(used.begin(), used.end());
    used.erase(std::unique(used.begin(), used.end()), used.end());
    for (hipEvent_t e : used) ctx->free_events.push_back(e);
    ctx->tail_event = nullptr; ctx->tail_fresh = false;
    SSW_TRY(base_prune_bill(ctx));
    return SSW_OK;
}

// Bases are generated on the context's stream, the stream every GEMM launch uses.
int get_basis(ssw_ctx* ctx, size_t n, bool inverse, bool f64, BasisKind kind, const void** out) {
    typedef BasisKind B;
    auto key = std::make_tuple(n, inverse, f64, kind);
    auto it = ctx->basis.find(key);
    if (it != ctx->basis.end()) { *out = it->second; return SSW_OK; }
    void* p = nullptr;
    if (kind != B::Dense && !f64) return SSW_ERR_BAD_ARG;
    const bool half = kind == B::HalfEven || kind == B::HalfOdd, rot = kind == B::Rot;
    // the split bases as dct_pair_prep.hip numbers them: cosE, sinE, cosO, sinO, and sinE for the launches
    const int split_which = kind == B::SinELaunch ? 4 : (int)kind - (int)B::CosE;
    const size_t elems = kind == B::Dense ? n * dense_basis_kpad(n)
                       : rot  ? n / 2
                       : half ? (n / 2) * dct_pair_kpad(n)
                              : dct_pair_split_basis_rows(n, split_which) * dct_pair_split_kpad(n);
    SSW_ALLOC(&p, std::max<size_t>(elems, 1) * (f64 ? sizeof(double) : sizeof(float)));
    int rc = rot  ? launch_make_rot_table(ctx->stream, n, (double*)p)
             : half ? launch_make_half_basis_blocked(ctx->stream, n, inverse, kind == B::HalfOdd ? 1 : 0, (double*)p)
             : kind != B::Dense ? launch_make_split_basis_blocked(ctx->stream, n, inverse, split_which, (double*)p)
             : f64  ? launch_make_basis_f64(ctx->stream, n, inverse, (double*)p)
                    : launch_make_basis_f32(ctx->stream, n, inverse, (float*)p);
    untimed_work(ctx);
    if (rc != SSW_OK) { (void)hipFree(p); return rc; }
    ctx->basis[key] = p;
    *out = p;
    return SSW_OK;
}

// Both bases of launch class `c` over a length-`len` axis as f16 hi + lo fragments for the pairs from pair0 on
// (base_energy.hip), cached in a map of their own and freed with the bases they are made from
int get_split16(ssw_ctx* ctx, size_t len, PairClass c, const double* y1, const double* y2, unsigned yrows, unsigned NP, unsigned Kp, unsigned pair0,
                const void** out) {
    auto key = std::make_tuple(len, (int)c, pair0);
    auto it = ctx->split16.find(key);
    if (it != ctx->split16.end()) { *out = it->second; return SSW_OK; }
    void* p = nullptr;
    SSW_ALLOC(&p, base_energy_split_bytes(NP, Kp, pair0));
    const int rc = launch_base_energy_split(ctx->stream, y1, y2, yrows, NP, Kp, pair0, p);
    untimed_work(ctx);
    if (rc != SSW_OK) { (void)hipFree(p); return rc; }
    ctx->split16[key] = p;
    *out = p;
    return SSW_OK;
}

bool valid_method(int m) { return m == SSW_OPTION1 || m == SSW_OPTION2 || m == SSW_OPTION3; }
bool valid_ordering(int o) { return o == SSW_ORDER_ENERGY || o == SSW_ORDER_ENERGY_ORTHOGONAL || o == SSW_ORDER_LEGACY; }
bool valid_precision(int p) { return p == SSW_PRECISION_F32 || p == SSW_PRECISION_F64; }

int check_config(const ssw_config* cfg) {
    if (!cfg) return SSW_ERR_BAD_ARG;
    if (cfg->method == SSW_METHOD_CUSTOM || cfg->ordering == SSW_ORDER_CUSTOM) return SSW_ERR_UNSUPPORTED;
    if (!valid_method(cfg->method) || !valid_ordering(cfg->ordering) || !valid_precision(cfg->precision))
        return SSW_ERR_BAD_ARG;
    return SSW_OK;
}

// Frames per internal pass: the caller's setting, or (0 = automatic, the default) about 2^30 pixels -- 128 4K
// frames, 514 full-HD ones, 32 8K ones -- capped where the f64 operand planes of a pass would pass 4 GB (the
// operand-ready GEMMs walk them with 32-bit offsets).  The GEMM grids then run ~64 rounds of blocks: against
// 2^28 pixels (16 rounds, the r1 default) the tails and first-tile latencies weigh 2.8 % less at 4K, 1.8 % at
// full HD, 1.4 % at 8K.  Workspace: up to 44 B/px of a pass per lane (r5: the fused forward transform keeps row and column operands side by side), sized for 288 GB of HBM -- and
// clamped to half of what the device can give right now (free memory + what the lanes already hold), so that
// a smaller device or a co-tenant (torch's caching allocator) gets smaller passes instead of an
// SSW_ERR_OUT_OF_MEMORY.
size_t effective_chunk(const ssw_ctx* ctx, size_t w, size_t h, size_t n_frames) {
    size_t c = ctx->chunk_frames;
    if (c == 0) {
        const size_t px = std::max<size_t>(w * h, 1);
        c = std::max<size_t>(1, ((size_t)1 << 30) / px);
        const size_t per_frame = dct_pair_operand_elems(1, w, h) * sizeof(double);
        if (per_frame) c = std::max<size_t>(1, std::min(c, (size_t)0xFFFFFFFFull / per_frame));
        if (c >= 16) c &= ~(size_t)7;              // whole groups of 8 frames (4K: 129 -> 128: the GEMM line tiles stay whole)
        c = std::min(c, std::max<size_t>(n_frames, 1));
        size_t free_b = 0, total_b = 0;
        DeviceGuard g(ctx->device);
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
            // half of what the device can give: free memory, what the lanes already hold, and the spare handle planes
            // (dev_malloc gives those back before it fails).  A clamp can turn a one-pass call into several passes,
            // i.e. into two lanes: budget for one lane first, then for the lane count the clamped pass size implies.
            const size_t budget = (free_b + lane_bytes_held(ctx) + ctx->plane_pool_bytes) / 2;
            size_t c1 = std::max<size_t>(1, std::min(c, budget / (44 * px)));
            if (ctx->overlap && n_frames > c1) c1 = std::max<size_t>(1, std::min(c1, budget / (2 * 44 * px)));
            c = c1;
        } else {
            (void)hipGetLastError();
        }
    }
    return std::min(c, std::max<size_t>(n_frames, 1));
}

// ---- the 2-D transform as a chain ---------------------------------------------------------------------
namespace {

bool aligned_planes(const float* a, const float* b) { return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15) == 0; }
// What the builders of a pass share: the pass, its plan and what both its stages account.  Held by value in the stages.
struct PassBuild {
    ssw_ctx* ctx; Xform x; PassPlan p;
    bool first_pass, is_row, inverse, from_rgb;
    size_t n, w, h, len, lines;
    const float* src; float* dst; Epilogue ep;
    int st_pass, st_main, st_prep;
    double px, prep_bytes, out_bpp;
    // algorithmic bytes of the pass's GEMM launches (ssw_ctx_get_traffic): the operand planes in (one double per pixel), the
    // f32 result out -- or, in the last pass of Writer::result, I and Q in and the RGB frame out -- plus `xch` bytes per
    // pixel that the dependent launches of an inverse pass write and read back as doubles (A1: 1 + 1, T2: 2 + 2, E: 4 + 4)
    double gemm_bytes(double xch) const { return px * (8.0 + xch + out_bpp); }
    double flop(PairClass c) const { return pair_class_flop(c, lines, len); }      // executed flop of one launch of class c
    // the row launches write the plane between the passes class-major; the column launches read operands of their own
    PairLayout gemm_layout() const { return is_row ? p.layout : PairLayout(); }
    int gemm(hipStream_t st, int nc, const PairClassDesc* d, double* tmp = nullptr, double* tmp_out = nullptr, const RgbSink* sink = nullptr,
             const PairLayout& lay = PairLayout()) const {
        return launch_dct_pair_gemm_multi_f64(st, is_row, inverse, nc, d, dst, tmp, n, w, h, ep, sink, tmp_out, lay);
    }
    // what the pass's pre-pass reads: the frames themselves (first pass from RGB: Y on the fly, I / Q out) or the f32 plane
    RowInput row_input() const { return from_rgb ? RowInput::rgb(x.rgb_fmt, x.rgb, x.iq_i, x.iq_q) : RowInput::plane(src); }
};

// The classes of one stage: one launch over all of them when the pass merges them, else class by class -- with the main-stage
// timer around the last one when the pass has one (st_main >= 0).
template <class Launch>
int launch_classes(ssw_ctx* ctx, hipStream_t st, bool merge, int nc, const PairClassDesc* d, Launch launch, int st_main = -1,
                   double f_main = 0.0) {
    if (merge) return launch(nc, d);
    for (int c = 0; c + 1 < nc; ++c) SSW_TRY(launch(1, &d[c]));
    if (st_main < 0) return launch(1, &d[nc - 1]);
    StageTimer tm(ctx, st_main, st, f_main);
    return launch(1, &d[nc - 1]);
}

// Writer::result: the last pass of an inverse transform (a column pass) converts to RGB in its epilogue
RgbSink rgb_sink(const PassBuild& b, bool* fused_rgb) {
    RgbSink sink;
    if (b.inverse && !b.first_pass && !b.is_row && b.x.rgb_out && b.x.iq_i && b.x.iq_q) {
        sink.iq_i = b.x.iq_i; sink.iq_q = b.x.iq_q; sink.rgb = b.x.rgb_out; sink.u8 = b.x.rgb_out_u8;
        if (fused_rgb) *fused_rgb = true;
    }
    return sink;
}

// The launch descriptor of class `c` over a length-`len` axis: the operand planes are the caller's, the cached bases the
// class table's (a shared operand's second product reads the second row block of the same basis plane: `pairs` lines further
// inside every k-block = 64 bytes per line).
int class_desc(ssw_ctx* ctx, size_t len, bool inverse, PairClass c, const double* x1, const double* x2, PairClassDesc& d) {
    const PairClassRow& r = pair_class_row(c);
    const void *y1 = nullptr, *y2 = nullptr;
    SSW_TRY(get_basis(ctx, len / r.ydiv, inverse, true, r.y1, &y1));
    if (r.samex) y2 = (const char*)y1 + (len / r.ldiv / r.np_div) * 64;
    else SSW_TRY(get_basis(ctx, len / r.ydiv, inverse, true, r.y2, &y2));
    d = {c, x1, x2, (const double*)y1, (const double*)y2};
    return SSW_OK;
}

// The split scratch of a pass (the lane's `deep` operand slot) as the deep pre-passes write it, planes by number (DESIGN
// §3): level 1 -- AS BD AD BS R1 R2, K8 wide, then AS2 BD2 AD2 BS2, K16 wide; level 2 -- sixteen planes K16 wide, in `l2`
// (the fused column pass reads them from the row launches' buffer).  `rot`: the rotation table of the axis.
struct PairPlanes {
    size_t bytes = 0, p8 = 0, p16 = 0;
    const void* rot = nullptr;
    double *sp = nullptr, *l2 = nullptr;
    size_t l2_plane = 0;
    const double* plane(bool level2, int j) const {
        return level2 ? l2 + (size_t)j * l2_plane : j < 6 ? sp + (size_t)j * p8 : sp + 6 * p8 + (size_t)(j - 6) * p16;
    }
};
int pair_planes(const PassBuild& b, ssw_ctx::Lane& ws, PairPlanes& pp) {
    pp.bytes = dct_pair_operand_elems(b.n, b.w, b.h) * sizeof(double);
    if (!b.p.split) return SSW_OK;
    SSW_TRY(get_basis(b.ctx, b.len, false, true, BasisKind::Rot, &pp.rot));
    SSW_TRY(ws.split_scratch(split_scratch_elems(b.n, b.w, b.h) * sizeof(double), &pp.sp));
    pp.l2 = pp.sp;
    pp.p8 = b.lines * dct_pair_split_kpad(b.len);
    pp.p16 = pp.l2_plane = b.lines * dct_pair_split_kpad(b.len / 2);
    return SSW_OK;
}
// class `c` of the pass on the planes the table names for it
int class_desc(const PassBuild& b, PairClass c, const double* x1, const double* x2, PairClassDesc& d) {
    return class_desc(b.ctx, b.len, b.inverse, c, x1, x2, d);
}
int deep_desc(const PassBuild& b, const PairPlanes& pp, bool level2, PairClass c, PairClassDesc& d) {
    const signed char* x = level2 ? pair_class_row(c).l2x : pair_class_row(c).l1x;
    if (x[0] < 0 || !pp.sp) return SSW_ERR_BAD_ARG;
    return class_desc(b, c, pp.plane(level2, x[0]), pp.plane(level2, x[1]), d);
}
int deep_descs(const PassBuild& b, const PairPlanes& pp, bool level2, std::initializer_list<PairClass> cls, PairClassDesc* d) {
    for (PairClass c : cls) SSW_TRY(deep_desc(b, pp, level2, c, *d++));
    return SSW_OK;
}
// the rotation tables of the half- and (level 2) quarter-length transforms
int deep_rot(const PassBuild& b, bool level2, const void** rot2, const void** rot3) {
    SSW_TRY(get_basis(b.ctx, b.len / 2, false, true, BasisKind::Rot, rot2));
    return level2 ? get_basis(b.ctx, b.len / 4, false, true, BasisKind::Rot, rot3) : SSW_OK;
}

// the odd half of the full-length transform from the operand plane `odd`: one launch, or rotate + two
struct OddHalfLaunch { PairClassDesc d[2]; int n = 0; double flop = 0.0; };
int odd_half(const PassBuild& b, const PairPlanes& pp, const double* odd, OddHalfLaunch& o) {
    if (!b.p.split) {
        o.n = 1; o.flop = b.flop(PairClass::OddHalf);
        return class_desc(b, PairClass::OddHalf, odd, odd, o.d[0]);
    }
    o.n = 2; o.flop = b.flop(PairClass::E) + b.flop(PairClass::O);
    return deep_descs(b, pp, false, {PairClass::E, PairClass::O}, o.d);
}
int odd_rotate(const PassBuild& b, const PairPlanes& pp, hipStream_t st, const double* odd) {
    return b.p.split ? launch_dct_pair_rotate(st, odd, (const double*)pp.rot, pp.sp, b.lines, b.len) : SSW_OK;
}
int odd_gemm(const PassBuild& b, const OddHalfLaunch& o, hipStream_t st, double* tmpE, const RgbSink* sink) {
    for (int c = 0; c < o.n; ++c) SSW_TRY(b.gemm(st, 1, &o.d[c], tmpE, nullptr, sink));
    return SSW_OK;
}

// ---- one builder per strategy (dct_plan.hpp) ----
int build_dense(const PassBuild& b, Chain& ch) {
    ssw_ctx* ctx = b.ctx;
    const void* b0 = nullptr;
    SSW_TRY(get_basis(ctx, b.len, b.inverse, b.x.precision == SSW_PRECISION_F64, BasisKind::Dense, &b0));
    const double flop = 2.0 * (double)b.lines * (double)b.len * (double)b.len;
    ch.push_back({false, [=](hipStream_t st) -> int {
        StageTimer t(ctx, b.st_pass, st, flop);
        t.traffic(b.px * 8.0);
        if (b.is_row) return launch_dct_rows(st, b.x.precision, b.src, b.dst, b.lines, b.w, b0, b.ep);
        return launch_dct_cols(st, b.x.precision, b.src, b.dst, b.n, b.w, b.h, b0, b.ep);
    }});
    return SSW_OK;
}

int build_pair_l1(const PassBuild& b, ssw_ctx::Lane& ws, Chain& ch) {
    ssw_ctx* ctx = b.ctx;
    PairPlanes pp;
    SSW_TRY(pair_planes(b, ws, pp));
    ssw_ctx::Lane::OneLevel o;
    SSW_TRY(ws.one_level(pp.bytes, o));
    double *x1 = o.s, *x2 = o.d;
    ch.push_back({true, [=](hipStream_t st) -> int {
        StageTimer t(ctx, SSW_STAGE_DCT_PREP, st, b.prep_bytes);
        return launch_dct_pair_prep(st, b.is_row, b.inverse, b.src, b.n, b.w, b.h, x1, x2);
    }});
    const double f_main = b.flop(PairClass::OneLevel);
    PairClassDesc d;
    SSW_TRY(class_desc(b, PairClass::OneLevel, x1, x2, d));
    ch.push_back({false, [=](hipStream_t st) -> int {
        StageTimer t(ctx, b.st_pass, st, f_main);
        t.traffic(b.gemm_bytes(0.0));
        StageTimer tm(ctx, b.st_main, st, f_main);
        return b.gemm(st, 1, &d);
    }});
    return SSW_OK;
}

int build_pair_two(const PassBuild& b, ssw_ctx::Lane& ws, Chain& ch, bool* fused_rgb) {
    ssw_ctx* ctx = b.ctx;
    PairPlanes pp;
    SSW_TRY(pair_planes(b, ws, pp));
    ssw_ctx::Lane::TwoLevel o;
    SSW_TRY(ws.two_level(pp.bytes, b.inverse, o));
    double *x2 = o.odd, *xx1 = o.ss, *xx2 = o.sd;      // D | O, SS | EE, SD | EO
    double* tmpE = o.even;                             // inverse: the even half E, unrounded
    ch.push_back({true, [=](hipStream_t st) -> int {
        StageTimer t(ctx, b.st_prep, st, b.prep_bytes);
        SSW_TRY(launch_dct_pair_prep4(st, b.is_row, b.inverse, b.row_input(), b.n, b.w, b.h, xx1, xx2, x2));
        return odd_rotate(b, pp, st, x2);
    }});
    OddHalfLaunch odd;
    PairClassDesc even;
    SSW_TRY(odd_half(b, pp, x2, odd));
    SSW_TRY(class_desc(b, PairClass::EvenHalf, xx1, xx2, even));
    const double f_main = odd.flop, f_all = f_main + b.flop(PairClass::EvenHalf);
    const RgbSink sink = rgb_sink(b, fused_rgb);
    ch.push_back({false, [=](hipStream_t st) -> int {
        StageTimer t(ctx, b.st_pass, st, f_all);
        t.traffic(b.gemm_bytes(b.inverse ? 8.0 : 0.0));          // inverse: the even half E out and in
        // even half: a half-length transform of S (forward) / of the even coefficients (inverse), folded again
        SSW_TRY(b.gemm(st, 1, &even, tmpE));
        StageTimer tm(ctx, b.st_main, st, f_main);
        return odd_gemm(b, odd, st, tmpE, sink.rgb ? &sink : nullptr);
    }});
    return SSW_OK;
}

// forward pass, three levels: x- (odd frequencies), S- (2 mod 4), (SSS, SS-) (0 and 4 mod 8); on a column pass (8K: 4320
// rows) the pre-pass transposes like the two-level one
int build_pair_three(const PassBuild& b, ssw_ctx::Lane& ws, Chain& ch) {
    ssw_ctx* ctx = b.ctx;
    PairPlanes pp;
    SSW_TRY(pair_planes(b, ws, pp));
    ssw_ctx::Lane::ThreeLevel o;
    SSW_TRY(ws.three_level(pp.bytes, o));
    double *d1 = o.odd, *d2 = o.s_minus, *r1 = o.r1, *r2 = o.r2;
    ch.push_back({true, [=](hipStream_t st) -> int {
        StageTimer t(ctx, b.st_prep, st, b.prep_bytes);
        if (!b.is_row) SSW_TRY(launch_dct_pair_prep8_cols(st, b.src, b.n, b.w, b.h, r1, r2, d2, d1));
        else SSW_TRY(launch_dct_pair_prep8_rows(st, b.row_input(), b.n, b.w, b.h, r1, r2, d2, d1));
        return odd_rotate(b, pp, st, d1);
    }});
    OddHalfLaunch odd;
    PairClassDesc r, m;
    SSW_TRY(odd_half(b, pp, d1, odd));
    SSW_TRY(class_desc(b, PairClass::R1R2, r1, r2, r));
    SSW_TRY(class_desc(b, PairClass::OddHalf2, d2, d2, m));
    const double f_main = odd.flop, f_all = f_main + b.flop(PairClass::R1R2) + b.flop(PairClass::OddHalf2);
    ch.push_back({false, [=](hipStream_t st) -> int {
        StageTimer t(ctx, b.st_pass, st, f_all);
        t.traffic(b.gemm_bytes(0.0));
        SSW_TRY(b.gemm(st, 1, &r));
        SSW_TRY(b.gemm(st, 1, &m));
        StageTimer tm(ctx, b.st_main, st, f_main);
        return odd_gemm(b, odd, st, nullptr, nullptr);
    }});
    return SSW_OK;
}

// The deep strategies: one pre-pass writes the operands of all launches (D and SD split, SS folded a third time); forward
// passes of 64-divisible (rows) / 16-divisible (columns) length, inverse ones of 128- / 16-divisible length.

// forward, level 1: five launches, sums of len/8 terms (the half-length split and R1 / R2 at len/16)
int build_deep(const PassBuild& b, ssw_ctx::Lane& ws, Chain& ch) {
    typedef PairClass C;
    ssw_ctx* ctx = b.ctx;
    PairPlanes pp;
    const void *rot2 = nullptr, *rot3 = nullptr;
    SSW_TRY(pair_planes(b, ws, pp));
    SSW_TRY(deep_rot(b, false, &rot2, &rot3));
    double* sp = pp.sp;
    ch.push_back({true, [=](hipStream_t st) -> int {
        StageTimer t(ctx, b.st_prep, st, b.prep_bytes);
        if (!b.is_row) return launch_dct_pair_prep16_cols(st, b.src, b.n, b.w, b.h, sp, (const double*)pp.rot, (const double*)rot2, nullptr, b.p.prep, b.p.layout);
        return launch_dct_pair_prep16_rows(st, b.row_input(), b.n, b.w, b.h, sp, (const double*)pp.rot, (const double*)rot2, nullptr, false);
    }});
    const double f_main = b.flop(C::O), f_all = f_main + b.flop(C::E) + b.flop(C::R1R2) + b.flop(C::E2) + b.flop(C::O2);
    // a single frame's launches are too small alone (class E of a 4K frame: 272 blocks for 512 slots): one launch over all classes
    std::array<PairClassDesc, 5> merged, single;
    SSW_TRY(deep_descs(b, pp, false, {C::R1R2, C::E2, C::O2, C::O, C::E}, merged.data()));
    SSW_TRY(deep_descs(b, pp, false, {C::R1R2, C::E2, C::O2, C::E, C::O}, single.data()));
    ch.push_back({false, [=](hipStream_t st) -> int {
        StageTimer t(ctx, b.st_pass, st, f_all);
        t.traffic(b.gemm_bytes(0.0));
        auto launch = [&](int nc, const PairClassDesc* d) { return b.gemm(st, nc, d, nullptr, nullptr, nullptr, b.gemm_layout()); };
        if (!b.p.merge) return launch_classes(ctx, st, false, 5, single.data(), launch, b.st_main, f_main);
        StageTimer tm(ctx, b.st_main, st, f_all);
        return launch(5, merged.data());
    }});
    return SSW_OK;
}

// LEVEL 2: every operand of the full-length split and of SS folds or rotates once more in the pre-pass (dct_pair_split.hpp,
// DeepPlanes): the eight launches of kLevel2Classes, len/16 terms over len/16 pairs each, 2/3 of the level-1 multiply-adds.  The
// "main" timer brackets ONE launch: O rotated "+" (level 1: class O of the full-length split).  FUSED: the row pre-pass orders
// its lines (frame, unit of the column fold, line of the unit), the row launches' epilogue (EPI_FWD_COLOP) rounds to f32 --
// the store between the passes, src/dct2d.rs:152-168 -- applies the column pre-pass's arithmetic and writes the sixteen
// column-operand planes; the column pass is its eight launches only (4 + 4 + 8 B/px of plane and pre-pass become 8).
//
// What every level-2 route shares, set up once per pass: the operand planes and rotation tables, on a fused transform the
// column-operand buffer and how a launch takes part (`fc`), the eight launch descriptors of kLevel2Classes, and the accounts
// of the pass's GEMM stage.
struct Level2Pass {
    bool fused = false;
    PairPlanes pp;
    const void *rot2 = nullptr, *rot3 = nullptr;
    FuseCols fc;
    double pad = 1.0;                              // the padding units' share of the flop
    double f_main = 0.0, f_all = 0.0, bytes = 0.0;
    float* out = nullptr;
    std::array<PairClassDesc, 8> d;
};
int level2_pass(const PassBuild& b, ssw_ctx::Lane& ws, Level2Pass& l2) {
    ssw_ctx* ctx = b.ctx;
    const size_t n = b.n, w = b.w, h = b.h;
    l2.fused = b.p.strategy == PassStrategy::FusedRows || b.p.strategy == PassStrategy::FusedCols;
    SSW_TRY(pair_planes(b, ws, l2.pp));
    SSW_TRY(deep_rot(b, true, &l2.rot2, &l2.rot3));
    l2.bytes = b.gemm_bytes(0.0);
    l2.out = b.dst;
    if (l2.fused) {
        const size_t cplane = n * w * dct_pair_split_kpad(h / 2);          // column operands: n w lines, K16(h) wide
        double* cop = nullptr;
        SSW_TRY(ws.column_operands(16 * cplane * sizeof(double), &cop));
        l2.fc = FuseCols{FUSE_COLS};
        if (!b.is_row) { l2.pp.l2 = cop; l2.pp.l2_plane = cplane; }
        else {
            const void *crot1 = nullptr, *crot2 = nullptr, *crot3 = nullptr;
            SSW_TRY(get_basis(ctx, h, false, true, BasisKind::Rot, &crot1));
            SSW_TRY(get_basis(ctx, h / 2, false, true, BasisKind::Rot, &crot2));
            SSW_TRY(get_basis(ctx, h / 4, false, true, BasisKind::Rot, &crot3));
            const size_t lpad = n * 16 * dct_pair_fused_units(h);           // unit-ordered, padded lines
            l2.pp.l2_plane = lpad * dct_pair_split_kpad(b.len / 2);
            l2.pad = (double)lpad / (double)(n * h);
            l2.fc = FuseCols{FUSE_ROWS_COP, cop, (const double*)crot1, (const double*)crot2, (const double*)crot3};
            l2.bytes = b.px * 16.0;                             // row operands in, column operands out
            l2.out = nullptr;
        }
    }
    l2.f_main = b.flop(PairClass::O5); l2.f_all = 8.0 * l2.f_main;         // (every class: the same pairs and sum length)
    for (int c = 0; c < 8; ++c) SSW_TRY(deep_desc(b, l2.pp, true, kLevel2Classes[c], l2.d[c]));
    return SSW_OK;
}
// the pass's pre-pass (a fused column pass has none: the row launches wrote its operands)
void push_level2_prep(const PassBuild& b, const Level2Pass& l2, Chain& ch) {
    if (l2.fused && !b.is_row) return;
    ssw_ctx* ctx = b.ctx;
    ch.push_back({true, [=](hipStream_t st) -> int {
        StageTimer t(ctx, b.st_prep, st, b.prep_bytes);
        const double *rot1 = (const double*)l2.pp.rot, *rot2 = (const double*)l2.rot2, *rot3 = (const double*)l2.rot3;
        if (!b.is_row) return launch_dct_pair_prep16_cols(st, b.src, b.n, b.w, b.h, l2.pp.sp, rot1, rot2, rot3, b.p.prep, b.p.layout);
        return launch_dct_pair_prep16_rows(st, b.row_input(), b.n, b.w, b.h, l2.pp.sp, rot1, rot2, rot3, true, l2.fused);
    }});
}
// the pass's GEMM stage: the eight launches, as `fc` says (null: not a fused transform)
int run_level2_gemm(const PassBuild& b, const Level2Pass& l2, const FuseCols* fc, hipStream_t st) {
    StageTimer t(b.ctx, b.st_pass, st, l2.f_all * l2.pad, b.p.merge ? b.st_main : -1);      // (merged: a single frame's eight classes in one launch)
    t.traffic(l2.bytes);
    auto launch = [&](int nc, const PairClassDesc* dd) {
        return launch_dct_pair_gemm_multi_f64(st, b.is_row, false, nc, dd, l2.out, nullptr, b.n, b.w, b.h, b.ep, nullptr, nullptr, b.gemm_layout(), fc);
    };
    return launch_classes(b.ctx, st, b.p.merge, 8, l2.d.data(), launch, b.st_main, l2.f_main * l2.pad);
}
int build_deep_l2(const PassBuild& b, ssw_ctx::Lane& ws, Chain& ch) {
    Level2Pass l2;
    SSW_TRY(level2_pass(b, ws, l2));
    push_level2_prep(b, l2, ch);
    ch.push_back({false, [=](hipStream_t st) -> int { return run_level2_gemm(b, l2, l2.fused ? &l2.fc : nullptr, st); }});
    return SSW_OK;
}

// ---- the base reader of a batch extract: the fused forward transform whose row launches add up the column
// energies (base_energy.hip) and whose column pass runs only where a column can hold one of the first k keys (base_prune.hip);
// build_base_reader puts the two passes together ----
typedef std::function<int(hipStream_t)> TailLaunch;

// Row pass: the pre-pass, then one stage that zeroes the energies and runs the eight exact energy launches -- or, with the
// low-precision tail bound (base_energy.hip), where base_tail_plan finds every class with more than one tile column: the bound
// kernel over the tail pairs and the energy launches on tile column 0 only (the head).  The exact launches of the other tile
// columns are then `tail`, each block gated on the flags: they wait for the decide kernel in the column pass's chain.  No such
// launches: `tail` is empty.
int build_base_rows(const PassBuild& b, const Level2Pass& l2, const BaseReaderArgs& a, Chain& ch, TailLaunch& tail) {
    ssw_ctx* ctx = b.ctx;
    const size_t n = b.n, w = b.w, h = b.h;
    tail = nullptr;
    push_level2_prep(b, l2, ch);
    FuseCols fe = l2.fc;
    fe.energy = a.energy;
    BaseTailPlan tp;
    if (tuning(TUNE_BASE_ENERGY_LOWP) != 0) SSW_TRY(base_tail_plan(b.len, b.gemm_layout(), tuning(TUNE_TILE48) != 0, tp));
    if (!tp.eligible) {
        fe.part = BasePart::EnergyRows;
        ch.push_back({false, [=](hipStream_t st) -> int {
            SSW_HIP_CHECK(hipMemsetAsync(a.energy, 0, n * w * sizeof(float), st));
            untimed_work(ctx);
            return run_level2_gemm(b, l2, &fe, st);
        }});
        return SSW_OK;
    }
    std::array<BaseEnergyClass, 8> be;
    for (int c = 0; c < 8; ++c) {
        const BaseTailPlan::Class& k = tp.cls[c];
        const PairClassDesc& d = l2.d[c];
        const void* y16 = nullptr;
        SSW_TRY(get_split16(ctx, b.len, d.cls, d.y1, d.y2, k.yrows, tp.NP, k.Kp, tp.pair0, &y16));
        be[c].x1 = d.x1; be[c].x2 = d.x2; be[c].y16 = y16;
        be[c].NP = tp.NP; be[c].Kp = k.Kp; be[c].pair0 = tp.pair0; be[c].pm = k.pm; be[c].c1 = k.c1; be[c].c2 = k.c2; be[c].gsh = k.gsh; be[c].e2off = k.e2off;
    }
    const size_t lpf = 16 * dct_pair_fused_units(h);
    const double head = (double)tp.pair0 / (double)tp.NP;
    const double bound_bytes = 8.0 * 2.0 * (double)tp.chunks * (double)(n * lpf) * (double)be[0].Kp * 8.0;
    fe.part = BasePart::HeadRows;
    ch.push_back({false, [=](hipStream_t st) -> int {
        SSW_HIP_CHECK(hipMemsetAsync(a.energy, 0, n * w * sizeof(float), st));
        untimed_work(ctx);
        {
            StageTimer tb(ctx, SSW_STAGE_DCT_PREP, st, bound_bytes);
            SSW_TRY(launch_base_energy_bound(st, 8, be.data(), n, w, h, lpf, b.ep.base, a.energy));
        }
        // (not billed to the main-launch stage: that figure stays the time and flop of one full launch, the writer's)
        StageTimer t(ctx, b.st_pass, st, l2.f_all * l2.pad * head);
        t.traffic(b.px * 8.0 * (1.0 + head));
        auto launch = [&](int nc, const PairClassDesc* dd) {
            return launch_dct_pair_gemm_multi_f64(st, true, false, nc, dd, l2.out, nullptr, n, w, h, b.ep, nullptr, nullptr, b.gemm_layout(), &fe);
        };
        return launch_classes(ctx, st, b.p.merge, 8, l2.d.data(), launch);
    }});
    FuseCols ft = l2.fc;
    ft.part = BasePart::TailRows; ft.need = a.need;
    ft.tail = a.counters ? &a.counters->tail_jobs : nullptr;       // the launches count their jobs, and bill them at these rates per pair
    ft.tail_flop = 4.0 * (double)lpf * (double)(b.len / 16); ft.tail_bytes = 16.0 * (double)h;
    tail = [=](hipStream_t st) -> int {
        auto launch = [&](int nc, const PairClassDesc* dd) {
            return launch_dct_pair_gemm_multi_f64(st, true, false, nc, dd, l2.out, nullptr, n, w, h, b.ep, nullptr, nullptr, b.gemm_layout(), &ft);
        };
        return launch_classes(ctx, st, b.p.merge, 8, l2.d.data(), launch);
    };
    return SSW_OK;
}

// Column pass.  Phase 1: tile 0 of every frame (one launch over the eight classes, a grid of 3 blocks per frame and class);
// decide; the row pass's `tail`, if it left one: the column operands of the needed tiles are complete before phase 2 reads
// them; phase 2: the tiles that can hold one of the first k keys.  The others are not written: whoever reads the plane
// afterwards goes by the flags (launch_topk's mask).  The host bills phase 1; phase 2's tiles are billed from the device
// counters when the timers are resolved (base_prune_bill).
int build_base_cols(const PassBuild& b, const Level2Pass& l2, const BaseReaderArgs& a, const TailLaunch& tail, Chain& ch) {
    ssw_ctx* ctx = b.ctx;
    const size_t n = b.n, w = b.w, h = b.h;
    const double tiles = (double)(w / SSW_BASE_PRUNE_TILE);
    BasePrune bp;
    bp.energy = a.energy; bp.need = a.need; bp.k = a.k; bp.ordering = a.ordering;
    if (a.counters) { bp.stats = &a.counters->tiles; bp.work = &a.counters->col_flop; }
    bp.tile_flop = l2.f_all / ((double)n * tiles);
    bp.tile_bytes = l2.bytes / ((double)n * tiles);
    bp.select_bytes = (double)h * SSW_BASE_PRUNE_TILE * 4.0;
    auto phase = [=](hipStream_t st, BasePart part) {
        FuseCols f2 = l2.fc;
        f2.part = part; f2.need = a.need;
        return launch_dct_pair_gemm_multi_f64(st, false, false, 8, l2.d.data(), l2.out, nullptr, n, w, h, b.ep, nullptr, nullptr, b.gemm_layout(), &f2);
    };
    ch.push_back({false, [=](hipStream_t st) -> int {
        StageTimer t(ctx, b.st_pass, st, l2.f_all / tiles);
        t.traffic(l2.bytes / tiles);
        return phase(st, BasePart::Phase1Cols);
    }});
    ch.push_back({true, [=](hipStream_t st) -> int {
        StageTimer t(ctx, SSW_STAGE_SELECT, st, (double)n * ((double)h * SSW_BASE_PRUNE_TILE + (double)w) * 4.0);
        return launch_base_prune_decide(st, l2.out, bp, n, w, h);
    }});
    if (tail)
        ch.push_back({false, [=](hipStream_t st) -> int {
            StageTimer t(ctx, SSW_STAGE_DCT_ROW, st, 0.0);
            return tail(st);
        }});
    ch.push_back({false, [=](hipStream_t st) -> int {
        StageTimer t(ctx, b.st_pass, st, 0.0);
        return phase(st, BasePart::Phase2Cols);
    }});
    return SSW_OK;
}

// Columns of 8- but not 16-divisible length (1080 rows): D split and SS folded a third time in one pre-pass, SD stays one
// launch (H/16 is not whole); behind a deep row pass the plane arrives class-major (the staged pre-pass reads it like the
// deep one).  Inverse: c[8q] / c[8q+4] -> T2, the whole c[4q+2] part + T2 -> E, the split odd part + E -> output.
int build_semi_deep(const PassBuild& b, ssw_ctx::Lane& ws, Chain& ch, bool* fused_rgb) {
    typedef PairClass C;
    ssw_ctx* ctx = b.ctx;
    const bool inv = b.inverse;
    PairPlanes pp;
    SSW_TRY(pair_planes(b, ws, pp));
    ssw_ctx::Lane::Exchange x{nullptr, nullptr, nullptr};
    if (inv) SSW_TRY(ws.inverse_exchange(pp.bytes, 0, 0, false, x));      // (whole operand planes)
    double *T2 = x.t2, *TE = x.even;
    double* sp = pp.sp;
    const double* rot = (const double*)pp.rot;
    ch.push_back({true, [=](hipStream_t st) -> int {
        StageTimer t(ctx, b.st_prep, st, b.prep_bytes);
        if (inv) return launch_dct_pair_prep16_inv_cols(st, b.src, b.n, b.w, b.h, sp, rot, rot, nullptr, b.p.prep, b.p.layout);
        return launch_dct_pair_prep16_cols(st, b.src, b.n, b.w, b.h, sp, rot, rot, nullptr, b.p.prep, b.p.layout);
    }});
    const RgbSink sink = rgb_sink(b, fused_rgb);
    PairClassDesc r1, sd, eo[2];
    SSW_TRY(deep_desc(b, pp, false, C::R1R2, r1));
    SSW_TRY(deep_desc(b, pp, false, C::OddHalf2, sd));
    SSW_TRY(deep_descs(b, pp, false, {C::E, C::O}, eo));
    const double f_sd = b.flop(C::OddHalf2);
    const double f_main = b.flop(C::E), f_all = f_main + b.flop(C::O) + b.flop(C::R1R2) + f_sd;
    ch.push_back({false, [=](hipStream_t st) -> int {
        StageTimer t(ctx, b.st_pass, st, f_all);
        t.traffic(b.gemm_bytes(inv ? 12.0 : 0.0));
        if (inv) {
            SSW_TRY(b.gemm(st, 1, &r1, T2));
            SSW_TRY(b.gemm(st, 1, &sd, T2, TE));
            return launch_classes(ctx, st, b.p.merge, 2, eo, [&](int nc, const PairClassDesc* d) { return b.gemm(st, nc, d, TE, nullptr, sink.rgb ? &sink : nullptr); });
        }
        if (b.p.merge) {      // the SD launch shares its image operand between its two products: another template instance
            SSW_TRY(b.gemm(st, 1, &sd));
            const PairClassDesc d[3] = {r1, eo[1], eo[0]};
            StageTimer tm(ctx, b.st_main, st, f_all - f_sd);
            return b.gemm(st, 3, d);
        }
        SSW_TRY(b.gemm(st, 1, &r1));
        SSW_TRY(b.gemm(st, 1, &sd));
        SSW_TRY(b.gemm(st, 1, &eo[1]));
        StageTimer tm(ctx, b.st_main, st, f_main);
        return b.gemm(st, 1, &eo[0]);
    }});
    return SSW_OK;
}

// The inverse the deep way: c[8q] / c[8q+4] -> T2, the split c[4q+2] part + T2 -> T (the even half E), then the split odd
// part + T -> the output; one pre-pass for all launches.  LEVEL 2, the transpose of the forward pass's: T2 = its even half A1
// (R1+ R1-) +/- its odd half (R2 rotated); E = T2 +/- the half-length odd part (AS2 BD2 | AD2 BS2); x = E +/- the odd part
// (AS+ BD- | AS- BD+ | O rotated "+" | "-"): 8/14 of the level-1 multiply-adds.  The row launches write (and exchange E) class-major.
int build_deep_inv(const PassBuild& b, ssw_ctx::Lane& ws, Chain& ch, bool* fused_rgb) {
    typedef PairClass C;
    ssw_ctx* ctx = b.ctx;
    const bool l2 = b.p.strategy == PassStrategy::DeepInvL2;
    const size_t len = b.len, lines = b.lines;
    PairPlanes pp;
    const void *rot2 = nullptr, *rot3 = nullptr;
    SSW_TRY(pair_planes(b, ws, pp));
    SSW_TRY(deep_rot(b, l2, &rot2, &rot3));
    ssw_ctx::Lane::Exchange x;
    SSW_TRY(ws.inverse_exchange(pp.bytes, lines, len, l2, x));
    // unrounded: the eighth-length even part (level 2: len/8 doubles per line), the quarter-length even half, the even half E
    double *A1 = x.a1, *T2 = x.t2, *TE = x.even;
    double* sp = pp.sp;
    const RgbSink sink = rgb_sink(b, fused_rgb);
    ch.push_back({true, [=](hipStream_t st) -> int {
        StageTimer t(ctx, b.st_prep, st, b.prep_bytes);
        if (!b.is_row) return launch_dct_pair_prep16_inv_cols(st, b.src, b.n, b.w, b.h, sp, (const double*)pp.rot, (const double*)rot2, (const double*)rot3,
                                                              b.p.prep, b.p.layout);
        return launch_dct_pair_prep16_inv_rows(st, b.src, b.n, b.w, b.h, sp, (const double*)pp.rot, (const double*)rot2, (const double*)rot3, b.p.prep);
    }});
    // the stages: (level 2: A1, then) T2, E from T2, the output from E
    PairClassDesc da{}, dt, d1[2], d0[4];
    if (l2) SSW_TRY(deep_desc(b, pp, true, C::R1A, da));
    SSW_TRY(deep_desc(b, pp, l2, l2 ? C::R2A : C::R1R2, dt));
    SSW_TRY(deep_descs(b, pp, l2, {C::E2, C::O2}, d1));
    if (l2) SSW_TRY(deep_descs(b, pp, true, {C::EE, C::EO, C::O5, C::O3}, d0));
    else SSW_TRY(deep_descs(b, pp, false, {C::E, C::O}, d0));
    const double f_all = l2 ? 8.0 * b.flop(C::O5) : b.flop(C::E) + b.flop(C::O) + b.flop(C::R1R2) + b.flop(C::E2) + b.flop(C::O2);
    const std::array<PairClassDesc, 2> s1{d1[0], d1[1]};
    const std::array<PairClassDesc, 4> s0{d0[0], d0[1], d0[2], d0[3]};
    ch.push_back({false, [=](hipStream_t st) -> int {
        StageTimer t(ctx, b.st_pass, st, f_all);
        t.traffic(b.gemm_bytes(l2 ? 14.0 : 12.0));
        const PairLayout lay = b.gemm_layout();
        if (l2) SSW_TRY(b.gemm(st, 1, &da, A1));
        SSW_TRY(l2 ? b.gemm(st, 1, &dt, A1, T2, nullptr, lay) : b.gemm(st, 1, &dt, T2));
        // (single frames: the classes of each dependent stage in one launch)
        SSW_TRY(launch_classes(ctx, st, b.p.merge, 2, s1.data(), [&](int nc, const PairClassDesc* d) { return b.gemm(st, nc, d, T2, TE, nullptr, lay); }));
        return launch_classes(ctx, st, b.p.merge, l2 ? 4 : 2, s0.data(),
                              [&](int nc, const PairClassDesc* d) { return b.gemm(st, nc, d, TE, nullptr, sink.rgb ? &sink : nullptr, lay); });
    }});
    return SSW_OK;
}

// One pass of the separable transform (src -> dst along rows or columns) as its builders see it: its plan and what its
// stages account.
int make_pass(ssw_ctx* ctx, const Xform& x, bool first_pass, bool is_row, const float* src, float* dst, Epilogue ep, PassBuild& b) {
    const PlanInput in{x.type, x.precision, x.n, x.w, x.h, x.full_h, x.natural_order, aligned_planes(src, dst), plan_settings(ctx)};
    b = PassBuild{ctx, x, plan_pass(in, first_pass, is_row), first_pass, is_row, x.type == SSW_DCT3, x.rgb && first_pass, x.n, x.w, x.h,
                  is_row ? x.w : x.h, is_row ? x.n * x.h : x.n * x.w, src, dst, ep};
    if (b.from_rgb && !(is_row && b.p.levels >= 2)) return SSW_ERR_BAD_ARG;      // can_fuse_rgb() checks the same conditions
    b.st_pass = is_row ? SSW_STAGE_DCT_ROW : SSW_STAGE_DCT_COL;
    b.st_main = is_row ? SSW_STAGE_DCT_ROW_MAIN : SSW_STAGE_DCT_COL_MAIN;
    b.st_prep = b.from_rgb ? SSW_STAGE_RGB_TO_YIQ : SSW_STAGE_DCT_PREP;
    b.px = (double)b.n * (double)b.w * (double)b.h;
    // algorithmic bytes of the pre-pass: the f32 plane (or the RGB frame) in, the operand planes (one double per pixel, whatever
    // the number of folding levels) and I / Q out
    b.prep_bytes = b.from_rgb ? b.px * (3.0 * (double)pix_bytes(x.rgb_fmt) + (x.iq_i ? 8.0 : 0.0) + 8.0) : b.px * (4.0 + 8.0);
    const bool sink_pass = b.inverse && !first_pass && !is_row && x.rgb_out && x.iq_i && x.iq_q;
    b.out_bpp = sink_pass ? 8.0 + 3.0 * (x.rgb_out_u8 ? 1.0 : 4.0) : 4.0;
    return SSW_OK;
}
// hints for the two-lane scheduler (run_pipeline_impl) on the stages the pass's builder appended, ch[first] on
void tag_pass_stages(const PassBuild& b, Chain& ch, size_t first) {
    for (size_t i = first; i < ch.size(); ++i) {
        if (!ch[i].hbm && b.is_row) ch[i].tag = 1;
        if (ch[i].hbm && b.is_row && b.first_pass && b.x.type != SSW_DCT3 && b.x.rgb) ch[i].tag = 2;
    }
}

// The pass appended to `ch`: the builder of the strategy its plan names.
int build_pass(ssw_ctx* ctx, ssw_ctx::Lane& ws, const Xform& x, bool first_pass, bool is_row, const float* src, float* dst,
               Epilogue ep, Chain& ch, bool* fused_rgb = nullptr) {
    PassBuild b;
    SSW_TRY(make_pass(ctx, x, first_pass, is_row, src, dst, ep, b));
    const size_t first = ch.size();
    typedef PassStrategy S;
    const S s = b.p.strategy;
    SSW_TRY(s == S::Dense                   ? build_dense(b, ch)
            : s == S::PairL1                ? build_pair_l1(b, ws, ch)
            : s == S::PairTwo               ? build_pair_two(b, ws, ch, fused_rgb)
            : s == S::PairThree             ? build_pair_three(b, ws, ch)
            : s == S::Deep                  ? build_deep(b, ws, ch)
            : s == S::SemiDeep || s == S::SemiDeepInv ? build_semi_deep(b, ws, ch, fused_rgb)
            : s == S::DeepInv || s == S::DeepInvL2    ? build_deep_inv(b, ws, ch, fused_rgb)
                                                      : build_deep_l2(b, ws, ch));        // DeepL2, FusedRows, FusedCols
    tag_pass_stages(b, ch, first);
    return SSW_OK;
}

}  // namespace

int build_transform(ssw_ctx* ctx, ssw_ctx::Lane& ws, const Xform& x, Chain& ch, bool* fused_rgb) {
    const bool f64 = (x.precision == SSW_PRECISION_F64);
    const size_t n = x.n, w = x.w, h = x.h;
    if (n == 0) return SSW_OK;
    const size_t max_frames = plan_frame_limit(plan_settings(ctx), f64, w, h);
    if (n > max_frames) {
        for (size_t f0 = 0; f0 < n; f0 += max_frames) {
            Xform s = x;
            s.n = std::min(max_frames, n - f0);
            s.data = x.data + f0 * w * h;
            s.tmp = x.tmp + f0 * w * h;
            if (x.rgb) s.rgb = static_cast<const char*>(x.rgb) + f0 * w * h * 3 * pix_bytes(x.rgb_fmt);
            if (x.iq_i) s.iq_i = x.iq_i + f0 * w * h;
            if (x.iq_q) s.iq_q = x.iq_q + f0 * w * h;
            if (x.rgb_out) s.rgb_out = static_cast<char*>(x.rgb_out) + f0 * w * h * 3 * (x.rgb_out_u8 ? 1 : sizeof(float));
            SSW_TRY(build_transform(ctx, ws, s, ch, fused_rgb));
        }
        return SSW_OK;
    }
    const bool rows_first = (w >= h);                                  // src/dct2d.rs:93-98
    Epilogue plain{1.f, 1.f};
    auto ortho = [&](size_t len) {                                      // src/dct2d.rs:154-155
        Epilogue e{std::sqrt(1.0f / (4.0f * (float)len)), std::sqrt(1.0f / (2.0f * (float)len))};
        return e;
    };
    Epilogue last = plain;
    if (x.type == SSW_DCT3) last.first = last.base = (float)4 / (float)(w * h);           // :213-217
    for (int pass = 0; pass < 2; ++pass) {
        const bool is_row = (pass == 0) ? rows_first : !rows_first;
        const float* src = (pass == 0) ? x.data : x.tmp;
        float* dst = (pass == 0) ? x.tmp : x.data;
        const Epilogue ep = (x.type == SSW_DCT2_ORTHOGONAL) ? ortho(is_row ? w : h) : (pass == 1 ? last : plain);
        SSW_TRY(build_pass(ctx, ws, x, pass == 0, is_row, src, dst, ep, ch, fused_rgb));
    }
    return SSW_OK;
}

namespace {
// the row pass of a forward transform of n frames between the planes a and b
PassPlan forward_rows_plan(const ssw_ctx* ctx, bool f64, size_t n, size_t w, size_t h, const float* a, const float* b) {
    return plan_pass({SSW_DCT2, f64 ? SSW_PRECISION_F64 : SSW_PRECISION_F32, n, w, h, 0, false, aligned_planes(a, b), plan_settings(ctx)}, true, true);
}
}  // namespace

// the row pass takes two folding levels or more (its pre-pass can read RGB) and the frames suit that pre-pass
bool can_fuse_rgb(const ssw_ctx* ctx, bool f64, size_t w, size_t h, const float* y, const float* tmp, const void* rgb, PixFmt fmt) {
    return forward_rows_plan(ctx, f64, 1, w, h, y, tmp).levels >= 2 && dct_pair_can_prep_from_rgb(w, h, rgb, fmt);
}

// Writer::new / Reader::base / Reader::derived: rgb -> Y (+ I, Q) -> forward 2-D DCT of Y into `y`.
// Where the default GEMM strategy applies (rows first, two folding levels on the row axis) the colour
// conversion is fused into the first operand pre-pass and the f32 Y plane is never materialised.
int build_forward_from_rgb(ssw_ctx* ctx, ssw_ctx::Lane& ws, int precision, const void* rgb, PixFmt fmt, size_t n, size_t w,
                           size_t h, float* y, float* i, float* q, float* tmp, Chain& ch) {
    const bool f64 = precision == SSW_PRECISION_F64;
    Xform x{SSW_DCT2, precision, n, w, h, y, tmp};
    if (can_fuse_rgb(ctx, f64, w, h, y, tmp, rgb, fmt)) {
        x.rgb = rgb; x.rgb_fmt = fmt; x.iq_i = i; x.iq_q = q;
        return build_transform(ctx, ws, x, ch);
    }
    const size_t npix = n * w * h;
    const double bytes = (double)npix * (3.0 * (double)pix_bytes(fmt) + (i ? 12.0 : 4.0));
    ch.push_back({true, [=](hipStream_t st) -> int {
        StageTimer t(ctx, SSW_STAGE_RGB_TO_YIQ, st, bytes);
        if (fmt == PixFmt::U8) return launch_rgb8_to_yiq(st, static_cast<const uint8_t*>(rgb), npix, y, i, q);
        if (fmt == PixFmt::U16) return launch_rgb16_to_yiq(st, static_cast<const uint16_t*>(rgb), npix, y, i, q);
        return launch_rgb_to_yiq(st, static_cast<const float*>(rgb), npix, y, i, q);
    }});
    return build_transform(ctx, ws, x, ch);
}

// Reader::base of a batch extract, whose plane feeds only the selection of the first k keys and reads at those indices: where
// the planner takes the fused forward transform for these frames, its row pass with the energies and its column pass in two
// phases (build_base_rows, build_base_cols); *mask = the flags the column pass leaves -- the tiles whose flag is 0 are NOT
// written, the selection reads by them.  Anywhere else the ordinary transform, and *mask = null.
int build_base_reader(ssw_ctx* ctx, ssw_ctx::Lane& ws, int precision, const void* rgb, PixFmt fmt, size_t n, size_t w, size_t h, float* y,
                      float* tmp, const BaseReaderArgs& a, Chain& ch, const unsigned** mask) {
    const bool f64 = precision == SSW_PRECISION_F64;
    *mask = nullptr;
    if (n > 0 && w >= h && n <= plan_frame_limit(plan_settings(ctx), f64, w, h) && can_fuse_rgb(ctx, f64, w, h, y, tmp, rgb, fmt)) {
        Xform x{SSW_DCT2, precision, n, w, h, y, tmp};
        x.rgb = rgb; x.rgb_fmt = fmt;
        PassBuild rows, cols;
        SSW_TRY(make_pass(ctx, x, true, true, y, tmp, Epilogue{1.f, 1.f}, rows));
        SSW_TRY(make_pass(ctx, x, false, false, tmp, y, Epilogue{1.f, 1.f}, cols));
        if (rows.p.strategy == PassStrategy::FusedRows && cols.p.strategy == PassStrategy::FusedCols) {
            Level2Pass lr, lc;
            TailLaunch tail;
            const size_t first = ch.size();
            SSW_TRY(level2_pass(rows, ws, lr));
            SSW_TRY(build_base_rows(rows, lr, a, ch, tail));
            tag_pass_stages(rows, ch, first);
            const size_t first_col = ch.size();
            SSW_TRY(level2_pass(cols, ws, lc));
            SSW_TRY(build_base_cols(cols, lc, a, tail, ch));
            tag_pass_stages(cols, ch, first_col);
            *mask = a.need;
            return SSW_OK;
        }
    }
    return build_forward_from_rgb(ctx, ws, precision, rgb, fmt, n, w, h, y, nullptr, nullptr, tmp, ch);
}

// The two passes of a rows-first forward transform from RGB as separate chains (single-image handles: the row pass
// of the top half of a frame runs while the bottom half is still crossing PCIe -- image rows are independent lines
// of a row pass, so any band of rows gives the values the whole frame gives).  `rows` consecutive image rows starting
// at `rgb` -> the same rows of the intermediate plane `tmp` (+ I, Q); then the column pass tmp -> y on the whole frame.
bool can_split_forward_rows(const ssw_ctx* ctx, bool f64, size_t w, size_t h, size_t bands, const float* y, const float* tmp, const void* rgb, PixFmt fmt) {
    return bands >= 2 && w >= h && h % 16 == 0 && h % bands == 0 && can_fuse_rgb(ctx, f64, w, h, y, tmp, rgb, fmt) &&
           can_fuse_rgb(ctx, f64, w, h / bands, y, tmp, rgb, fmt);
}
int build_forward_rows_band(ssw_ctx* ctx, ssw_ctx::Lane& ws, int precision, const void* rgb, PixFmt fmt, size_t w, size_t rows,
                            size_t frame_h, float* tmp, float* i, float* q, Chain& ch) {
    Xform x{SSW_DCT2, precision, 1, w, rows, tmp /* never read or written by this pass */, tmp};
    x.rgb = rgb; x.rgb_fmt = fmt; x.iq_i = i; x.iq_q = q;
    x.full_h = frame_h;
    return build_pass(ctx, ws, x, true, true, tmp, tmp, Epilogue{1.f, 1.f}, ch);
}
int build_forward_cols_after_rows(ssw_ctx* ctx, ssw_ctx::Lane& ws, int precision, size_t w, size_t h, float* tmp, float* y, Chain& ch) {
    Xform x{SSW_DCT2, precision, 1, w, h, y, tmp};
    x.full_h = h;            // the row pass ran band by band through the f32 plane: the column pass reads it back (no fused operands)
    return build_pass(ctx, ws, x, false, false, tmp, y, Epilogue{1.f, 1.f}, ch);
}

int run_serial(Chain& ch, hipStream_t st) {
    for (auto& s : ch) SSW_TRY(s.run(st));
    return SSW_OK;
}

int dct2d_planes(ssw_ctx* ctx, int type, int precision, size_t n, size_t w, size_t h, float* data, float* tmp) {
    Chain ch;
    Xform x{type, precision, n, w, h, data, tmp};
    SSW_TRY(build_transform(ctx, ctx->lane[0], x, ch));
    return run_serial(ch, ctx->stream);
}

int topk(ssw_ctx* ctx, hipStream_t st, SelectWorkspace& sel, const float* coef, size_t n, size_t w, size_t h, int ordering,
         size_t k, uint32_t* idx, const unsigned* need) {
    // (under a tile mask: tile 0 of every frame; the other needed tiles are billed from the device counters, base_prune_bill)
    const double bytes = 4.0 * (double)n * (double)(need ? SSW_BASE_PRUNE_TILE : w) * (double)h;
    if (need && k > select_max_k()) return SSW_ERR_BAD_ARG;
    if (k > select_max_k()) {
        // Beyond the in-LDS top-k limit (16384 entries; BASELINE marks are 1000 and 10000 long): the full order of
        // every plane (sort_full.hip: a batched radix sort over all frames of the call), first k entries kept.  Off
        // the hot path: only Reader::indices() with a large k and marks that long reach it.
        size_t sb = 0;
        SSW_TRY(full_sort_scratch_bytes(w * h, n, &sb));
        SSW_TRY(grow(ctx->shared.sort_scratch, sb));
        StageTimer t(ctx, SSW_STAGE_SELECT, st, bytes);
        return launch_full_sort(st, coef, n, w, h, ordering, ctx->shared.sort_scratch.p, ctx->shared.sort_scratch.bytes, idx, k);
    }
    SSW_TRY(grow_select(st, sel, n, k));
    sel.fallbacks = ctx->select_fallbacks;
    ctx->select_frames += n;
    StageTimer t(ctx, SSW_STAGE_SELECT, st, bytes);
    return launch_topk(st, coef, n, w, h, ordering, k, sel, idx, need, need ? SSW_BASE_PRUNE_TILE : 0u);
}

// ---- two-lane pipeline ----------------------------------------------------------------------------------
namespace {

int next_sync_event(ssw_ctx* ctx, hipEvent_t* out) {
    constexpr size_t RING = 256;
    if (ctx->sync_events.size() < RING) {
        hipEvent_t e = nullptr;
        SSW_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        ctx->sync_events.push_back(e);
        *out = e;
        return SSW_OK;
    }
    *out = ctx->sync_events[ctx->sync_next % RING];
    ctx->sync_next++;
    return SSW_OK;
}

// A lane's stage has just been enqueued on ln.cur: remember that point (an event recorded NOW -- recorded
// later it would also cover what the other lane has enqueued on the same stream in the meantime, and the
// lanes would serialise each other).
int mark_done(ssw_ctx* ctx, ssw_ctx::Lane& ln) {
    SSW_TRY(next_sync_event(ctx, &ln.done));
    SSW_HIP_CHECK(hipEventRecord(ln.done, ln.cur));
    untimed_work(ctx);
    return SSW_OK;
}

// continue the lane's chain on stream `to`: the lane's last stage happens before
int hop(ssw_ctx* ctx, ssw_ctx::Lane& ln, hipStream_t to) {
    if (ln.cur == to) return SSW_OK;
    if (ln.done) SSW_HIP_CHECK(hipStreamWaitEvent(to, ln.done, 0));
    untimed_work(ctx);                             // the next stage's timer starts behind the wait, not in front of it
    ln.cur = to;
    return SSW_OK;
}

bool pipeline_uses_two_lanes(const ssw_ctx* ctx, size_t n_chunks) {
    // from two passes on (r3: with the pre-passes a quarter of a pass, the second lane's pre-passes fill the gaps between
    // the first lane's GEMM launches: +2.1 % at 2 x 128 4K frames; r2 measured nothing below three passes)
    return ctx->overlap && n_chunks >= 2 && ctx->aux_stream != nullptr;
}

// Runs build(chunk, lane, chain) for every chunk and enqueues the chains: one lane on one stream when
// overlap is off, else two lanes round-robin with GEMM stages on ctx->stream and HBM-bound stages on
// ctx->aux_stream.  On return the context's stream is ordered after everything that was enqueued.
int run_pipeline_impl(ssw_ctx* ctx, size_t n_chunks, bool two, const std::function<int(size_t, ssw_ctx::Lane&, Chain&)>& build) {
    hipStream_t G = ctx->stream, H = two ? ctx->aux_stream : ctx->stream;
    const int n_lanes = two ? 2 : 1;
    if (two) {                                     // the caller's earlier work on the context's stream comes first
        hipEvent_t ev = nullptr;
        SSW_TRY(next_sync_event(ctx, &ev));
        SSW_HIP_CHECK(hipEventRecord(ev, G));
        SSW_HIP_CHECK(hipStreamWaitEvent(H, ev, 0));
        untimed_work(ctx);
    }
    Chain chain[ssw_ctx::MAX_LANES];
    size_t at[ssw_ctx::MAX_LANES] = {0, 0};
    bool active[ssw_ctx::MAX_LANES] = {false, false};
    size_t next = 0;
    auto start = [&](int l) -> int {
        active[l] = false;
        while (next < n_chunks) {
            chain[l].clear();
            at[l] = 0;
            const size_t bases = ctx->basis.size();
            SSW_TRY(build(next++, ctx->lane[l], chain[l]));
            if (two && ctx->basis.size() != bases) {
                // get_basis made a missing table on the context's stream while the chain was built: the stages that run on
                // the second stream (an RGB pre-pass reads the rotation tables) must not start before it is written
                hipEvent_t ev = nullptr;
                SSW_TRY(next_sync_event(ctx, &ev));
                SSW_HIP_CHECK(hipEventRecord(ev, G));
                SSW_HIP_CHECK(hipStreamWaitEvent(H, ev, 0));
                untimed_work(ctx);
            }
            if (!chain[l].empty()) { active[l] = true; break; }
        }
        return SSW_OK;
    };
    for (int l = 0; l < n_lanes; ++l) {
        ctx->lane[l].cur = H;
        ctx->lane[l].done = nullptr;
        SSW_TRY(start(l));
    }
    // `lane_stagger` (r5 experiment): the second lane starts one stage late, and an RGB pre-pass waits until the other lane's
    // row pass is through -- it then runs beside that lane's COLUMN launches (MFMA-bound, 12 B/px) instead of its row
    // launches (16 B/px and an epilogue that is HBM-bound itself)
    const bool stagger = two && tuning(TUNE_LANE_STAGGER) != 0;
    bool held_back = stagger;
    while (active[0] || active[1]) {
        for (int l = 0; l < n_lanes; ++l) {
            if (!active[l]) continue;
            if (l == 1 && held_back) { held_back = false; continue; }
            Stage& s = chain[l][at[l]];
            SSW_TRY(hop(ctx, ctx->lane[l], s.hbm ? H : G));
            if (stagger && s.tag == 2) {
                const int o = 1 - l;
                if (active[o] && at[o] > 0 && chain[o][at[o] - 1].tag == 1 && ctx->lane[o].done)
                    SSW_HIP_CHECK(hipStreamWaitEvent(ctx->lane[l].cur, ctx->lane[o].done, 0));
                untimed_work(ctx);
            }
            SSW_TRY(s.run(ctx->lane[l].cur));
            if (two) SSW_TRY(mark_done(ctx, ctx->lane[l]));
            if (++at[l] == chain[l].size()) SSW_TRY(start(l));
        }
    }
    for (int l = 0; l < n_lanes; ++l) SSW_TRY(hop(ctx, ctx->lane[l], G));
    return SSW_OK;
}

int run_pipeline(ssw_ctx* ctx, size_t n_chunks, const std::function<int(size_t, ssw_ctx::Lane&, Chain&)>& build) {
    if (n_chunks == 0) return SSW_OK;
    // two lanes pay from three chunks on (with two, each lane would run a single chunk: measured equal to one lane)
    const bool two = pipeline_uses_two_lanes(ctx, n_chunks);
    int rc = run_pipeline_impl(ctx, n_chunks, two, build);
    if (rc == SSW_ERR_OUT_OF_MEMORY && !ctx->retired.empty()) {
        // Workspaces that grew during this call left their old allocations retired (grow(): stages already built may hold
        // them), so the call's peak was old + new.  Everything enqueued so far is complete after the waits below and nothing
        // built is still to run: give the retired buffers back and run the chunks again (same kernels, same outputs).
        if (two) (void)hipStreamSynchronize(ctx->aux_stream);
        (void)hipStreamSynchronize(ctx->stream);
        for (void* p : ctx->retired) (void)hipFree(p);
        ctx->retired.clear();
        untimed_work(ctx);
        rc = run_pipeline_impl(ctx, n_chunks, two, build);
    }
    if (rc != SSW_OK && two) {
        // a failing stage (out of memory inside grow(), most likely) must not leave the second stream running
        // behind the caller's back: the lanes' buffers are reused by the next call on the context's stream
        (void)hipStreamSynchronize(ctx->aux_stream);
        (void)hipStreamSynchronize(ctx->stream);
    }
    return rc;
}

// ---- pruned transform of the derived frames (prune.hip) ---------------------------------------
struct PruneSetup {
    bool on = false;
    PrunePlan plan;
    PassPlan rows;                  // of the full transform's row pass: levels 2 or 3; the split odd half (two classes instead
                                    // of one); deep: frequencies 2 mod 4 split as well, 0 / 4 mod 8 from the third level
    PruneClassSrc src[9];           // per class of `plan`: what its subset product reads (dct_pair_class.hpp)
    size_t gathered_bytes = 0;      // of one order of the gathered bases; 0: the class table does not serve this length (the chain fails)
};

// capacity of the compact plane in frequency columns: the index lists of natural spectra use ~3 sqrt(k)
// distinct columns (measured: 80..110 for k = 1000 at full HD and 4K); 8 sqrt(k), split over the classes
// in proportion to their share of all frequencies, leaves a wide margin, and a chunk that does not fit is
// redone with the full transform.
size_t prune_capacity(size_t k) {
    size_t c = (size_t)std::ceil(8.0 * std::sqrt((double)k));
    c = (c + 31) / 32 * 32;
    return std::max<size_t>(c, 64);
}

PruneSetup make_prune_setup(const ssw_ctx* ctx, bool f64, size_t n, size_t w, size_t h, size_t k, const float* y, const float* tmp,
                            const void* rgb, PixFmt fmt) {
    PruneSetup ps;
    if (!ctx->prune || k == 0 || !f64) return ps;                          // (the pair path runs in f64 only)
    if (!can_fuse_rgb(ctx, f64, w, h, y, tmp, rgb, fmt)) return ps;       // rows first, >= two folding levels on the rows
    const bool aligned = aligned_planes(y, tmp);
    if (!dct_pair_can_run(n, w, h, aligned)) return ps;                   // the chunk's planes within the 4 GB walk
    const size_t cap = prune_capacity(k);
    if (cap * 4 > w) return ps;                                           // not worth it: full transform
    if (!dct_pair_can_run(n, cap, h, aligned)) return ps;
    ps.rows = forward_rows_plan(ctx, f64, n, w, h, y, tmp);
    ps.plan.W = (unsigned)w;
    ps.plan.cap_total = (unsigned)cap;
    PairClass cls[8];
    const int n_cls = prune_class_list(ps.rows, cls);             // the row pass's launch classes: one list feeds the plan and its sources
    prune_plan_classes(cls, n_cls, (unsigned)cap, ps.plan);
    if (prune_class_sources(cls, n_cls, ps.rows, w, ps.src) != 0) ps.gathered_bytes = prune_gathered_offsets(ps.plan, ps.src);
    ps.on = true;
    return ps;
}

// The pruned path ends with one look at the overflow flags on the host; a stream that is being captured into
// a graph cannot be waited for, so such a call takes the full transform (enqueue-only, no host round trip).
bool stream_capturing(ssw_ctx* ctx) {
    hipStreamCaptureStatus capture = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(ctx->stream, &capture) != hipSuccess) { (void)hipGetLastError(); capture = hipStreamCaptureStatusNone; }
    return capture != hipStreamCaptureStatusNone;
}

// One class of the plan with its pointers; the launches' per-class arguments are each one conversion of it
struct PrunedClass {
    PruneClassSrc s;                               // planes by number (the fused kernel's A-fragments), sum lengths, gathered offsets
    const double *x = nullptr, *x2 = nullptr;      // operand plane(s) (set per chunk; x2: the sine operand of a split class)
    const void *basis = nullptr, *basis2 = nullptr;      // cached bases (basis2: split only)
};
// The prune tables: the column set of one or more index lists (launch_prune_build) and the rows of the cached bases gathered
// for it.  Three owners: a chunk of batch extract (its lane's buffers), the single-image handle (lane 0's), and a whole
// trace call (the context's: every chunk on both lanes reads ONE list, so they are made once before the pipeline starts).
struct PruneTables {
    PrunePlan plan;
    PassPlan rows;                                 // the row pass the plan prunes
    uint32_t *flag, *pos, *rows_of, *info;         // [W] | [W] | [cap_total] | the info block: overflow flag, columns per class
    char *gathered, *gathered_frag;                // the bases in launch order | in the fused pass's fragment order
    const double* rot[3];                          // rotation tables of the split row pass: of w, w / 2, w / 4
    PrunedClass c[9];
    const double* y(unsigned i, bool frag, bool second) const {
        if (second && !c[i].s.split) return nullptr;
        return (const double*)((frag ? gathered_frag : gathered) + (second ? c[i].s.goff2 : c[i].s.goff));
    }
    DerivedFusedClass fused(unsigned i) const {
        return {y(i, true, false), y(i, true, true), (unsigned)c[i].s.p1, (unsigned)(c[i].s.p2 < 0 ? 0 : c[i].s.p2), plan.c[i].cap, plan.c[i].off, c[i].s.split};
    }
    PairSubsetClass subset(unsigned i) const { return {c[i].x, c[i].x2, y(i, false, false), y(i, false, true), plan.c[i].cap, c[i].s.Kp, plan.c[i].off}; }
    PruneGatherJob gather(unsigned i, bool frag, bool second) const {
        return {rows_of + plan.c[i].off, (const char*)(second ? c[i].basis2 : c[i].basis), (char*)y(i, frag, second), plan.c[i].cap, c[i].s.src_rows,
                (unsigned)(c[i].s.Kp / KBlock<double>::KB), 0u, second, frag};
    }
};

// Lays the tables out in their owner's buffers -- `lane`, or the context (null) -- and resolves the plan's bases.  A lane's two
// orders of the gathered bases share one buffer (a chunk takes one row route); a call's keep both: its last chunk may take the other.
int lay_out_prune_tables(ssw_ctx* ctx, ssw_ctx::Lane* lane, const PruneSetup& ps, size_t w, uint32_t* info, PruneTables& t) {
    const bool deep = plan_is_deep(ps.rows), level2 = plan_is_level2(ps.rows);
    if ((deep && !ps.rows.split) || ps.gathered_bytes == 0) return SSW_ERR_BAD_ARG;
    PruneBufs& pb = lane ? lane->prune : ctx->trace.prune;
    ssw_ctx::Buf &u32 = pb.u32, &natural = pb.gathered, &frag = lane ? pb.gathered : pb.gathered_frag;
    t.plan = ps.plan;
    t.rows = ps.rows;
    t.info = info;
    SSW_TRY(grow(u32, (2 * w + ps.plan.cap_total + 64) * sizeof(uint32_t)));
    t.flag = u32.as<uint32_t>();
    t.pos = t.flag + w;
    t.rows_of = t.pos + w;
    t.rot[0] = t.rot[1] = t.rot[2] = nullptr;
    if (ps.rows.split) {
        SSW_TRY(get_basis(ctx, w, false, true, BasisKind::Rot, (const void**)&t.rot[0]));
        if (deep) SSW_TRY(get_basis(ctx, w / 2, false, true, BasisKind::Rot, (const void**)&t.rot[1]));
        if (level2) SSW_TRY(get_basis(ctx, w / 4, false, true, BasisKind::Rot, (const void**)&t.rot[2]));
    }
    for (unsigned i = 0; i < ps.plan.n_classes; ++i) {
        t.c[i] = PrunedClass();
        t.c[i].s = ps.src[i];
        SSW_TRY(get_basis(ctx, w / ps.src[i].ydiv, false, true, ps.src[i].y1, &t.c[i].basis));
        if (ps.src[i].split) SSW_TRY(get_basis(ctx, w / ps.src[i].ydiv, false, true, ps.src[i].y2, &t.c[i].basis2));
    }
    SSW_TRY(grow(natural, ps.gathered_bytes));
    if (!lane && level2) SSW_TRY(grow(frag, ps.gathered_bytes));
    t.gathered = natural.as<char>();
    t.gathered_frag = frag.as<char>();
    return SSW_OK;
}

// The one place the tables are made: the column set of `n_lists` index lists (idx null: this chain built it in an earlier
// stage), then the bases' rows in launch order and / or in fragment order.
int enqueue_prune_tables(hipStream_t st, const PruneTables& t, const uint32_t* idx, size_t n_lists, size_t k, bool want_natural, bool want_frag) {
    if (idx) SSW_TRY(launch_prune_build(st, idx, n_lists, k, t.plan, t.flag, t.rows_of, t.pos, t.info));
    for (bool frag : {false, true}) {
        if (!(frag ? want_frag : want_natural)) continue;
        PruneGatherJobs jobs;
        jobs.n = 0;
        for (unsigned i = 0; i < t.plan.n_classes; ++i) {
            jobs.j[jobs.n++] = t.gather(i, frag, false);
            if (t.c[i].s.split) jobs.j[jobs.n++] = t.gather(i, frag, true);
        }
        SSW_TRY(launch_prune_gather_bases(st, jobs));
    }
    return SSW_OK;
}

// the tables of a whole call (one index list), in the context, enqueued on its stream before the pipeline starts
int make_call_prune_tables(ssw_ctx* ctx, const PruneSetup& ps, size_t w, size_t k, const uint32_t* idx, uint32_t* info) {
    PruneTables t;
    SSW_TRY(lay_out_prune_tables(ctx, nullptr, ps, w, info, t));
    untimed_work(ctx);
    return enqueue_prune_tables(ctx->stream, t, idx, 1, k, true, plan_is_level2(ps.rows));
}

// what the route builders of one chunk share; held by value in the stages
struct PrunedChunk {
    ssw_ctx* ctx;
    RowInput in;                    // the derived frames: an RGB source, no I / Q out
    size_t n, w, h, k, lines;
    const uint32_t* idx;
    bool make_tables;               // this chain makes the tables it reads (else the call did: make_call_prune_tables)
    double *sp, *o[4];              // the split scratch and the lane's four planes of the folded pre-passes, o[PruneClassSrc::lane_buf]
    float* t_compact;               // the row pass's output [lines][cap]
    PruneTables t;
    size_t cap() const { return t.plan.cap_total; }
    double px() const { return (double)n * (double)w * (double)h; }
    double rgb_bytes() const { return px() * 3.0 * (double)pix_bytes(pix_fmt(in.kind)); }      // the frames, once in
};

// r5: marks of up to 1024 entries at level 2 -- the whole row pass in one kernel (dct_pair_derived.hip): no operand planes.
// A chain that makes its tables does so in one HBM stage in front of it.
void pruned_rows_fused(const PrunedChunk& q, const std::array<DerivedFusedClass, 9>& fca, Chain& ch) {
    ssw_ctx* ctx = q.ctx;
    if (q.make_tables)
        ch.push_back({true, [=](hipStream_t st) -> int {
            untimed_work(ctx);
            return enqueue_prune_tables(st, q.t, q.idx, q.n, q.k, false, true);
        }});
    const double in_bytes = q.rgb_bytes();
    // (timed with the RGB pre-passes: an HBM-bound kernel -- frames in, compact plane out -- whose 0.1e12 flop ride along;
    // bench.py's GEMM family stays "every pair_gemm_f64_kernel launch")
    ch.push_back({false, [=](hipStream_t st) -> int {
        StageTimer t(ctx, SSW_STAGE_RGB_TO_YIQ, st, in_bytes + (double)q.lines * (double)q.cap() * 4.0);
        return launch_dct_pair_derived_fused(st, q.in, q.lines, q.w, q.t.rot[0], q.t.rot[1], q.t.rot[2], q.t.plan.n_classes, fca.data(),
                                             q.t_compact, (unsigned)q.cap());
    }});
}

// Reader::derived's colour conversion + operand pre-pass (same kernels as the full path), then the subset products.  A chain
// that makes its tables builds the column set in front of the pre-pass and gathers in front of the products: two streams.
void pruned_rows_gathered(const PrunedChunk& q, Chain& ch) {
    ssw_ctx* ctx = q.ctx;
    const bool deep = plan_is_deep(q.t.rows), level2 = plan_is_level2(q.t.rows);
    const int levels = q.t.rows.levels;
    const unsigned ncl = q.t.plan.n_classes;
    const double prep_bytes = q.rgb_bytes() + q.px() * 8.0;
    double flop = 0.0;
    for (unsigned c = 0; c < ncl; ++c) flop += (q.t.c[c].s.split ? 4.0 : 2.0) * (double)q.lines * q.t.plan.c[c].cap * (double)q.t.c[c].s.ktrue;
    ch.push_back({true, [=](hipStream_t st) -> int {
        if (q.make_tables) {
            SSW_TRY(enqueue_prune_tables(st, q.t, q.idx, q.n, q.k, false, false));
            untimed_work(ctx);
        }
        StageTimer t(ctx, SSW_STAGE_RGB_TO_YIQ, st, prep_bytes);
        if (deep) return launch_dct_pair_prep16_rows(st, q.in, q.n, q.w, q.h, q.sp, q.t.rot[0], q.t.rot[1], q.t.rot[2], level2);
        if (levels == 3) SSW_TRY(launch_dct_pair_prep8_rows(st, q.in, q.n, q.w, q.h, q.o[2], q.o[3], q.o[0], q.o[1]));
        else SSW_TRY(launch_dct_pair_prep4(st, true, false, q.in, q.n, q.w, q.h, q.o[2], q.o[3], q.o[1]));
        return q.sp ? launch_dct_pair_rotate(st, q.o[1], q.t.rot[0], q.sp, q.lines, q.w) : SSW_OK;
    }});
    ch.back().tag = 2;
    ch.push_back({false, [=](hipStream_t st) -> int {
        if (q.make_tables) {
            SSW_TRY(enqueue_prune_tables(st, q.t, nullptr, 0, 0, true, false));
            untimed_work(ctx);
        }
        StageTimer t(ctx, SSW_STAGE_DCT_ROW, st, flop);
        t.traffic(q.px() * 8.0 + (double)q.lines * (double)q.cap() * 4.0);      // every operand plane once in, the compact plane out
        if (plan_merge(q.lines)) {          // a single frame: the classes side by side in one launch per kind
            PairSubsetClass sc[9];
            for (unsigned c = 0; c < ncl; ++c) sc[c] = q.t.subset(c);
            return launch_dct_pair_gemm_rows_subset_merged_f64(st, sc, ncl, q.t_compact, (unsigned)q.cap(), q.lines);
        }
        for (unsigned c = 0; c < ncl; ++c) {
            const PairSubsetClass s = q.t.subset(c);
            if (s.x2) SSW_TRY(launch_dct_pair_gemm_rows_subset_split_f64(st, s.x1, s.x2, s.y1, s.y2, s.cap, s.Kp, q.t_compact, (unsigned)q.cap(), s.off, q.lines));
            else SSW_TRY(launch_dct_pair_gemm_rows_subset_f64(st, s.x1, s.y1, s.cap, s.Kp, q.t_compact, (unsigned)q.cap(), s.off, q.lines));
        }
        return SSW_OK;
    }});
}

// column pass on the compact plane: the second pass of the same transform, `cap` columns wide, into ws.compact.cols
int pruned_cols(ssw_ctx* ctx, ssw_ctx::Lane& ws, size_t n, size_t cap, size_t h, Chain& ch) {
    float *t_compact = ws.compact.rows.as<float>(), *compact = ws.compact.cols.as<float>();
    Xform xc{SSW_DCT2, SSW_PRECISION_F64, n, cap, h, compact, t_compact};
    xc.natural_order = true;                 // the compact plane's columns are the gathered frequencies, in the plan's order
    return build_pass(ctx, ws, xc, false, false, t_compact, compact, Epilogue{1.f, 1.f}, ch);
}

// derived rgb frames -> compact coefficient plane ws.compact.cols [n][h][cap_total] holding, for every frequency column the
// index lists use, the column the full (f64: make_prune_setup) transform would produce.  `call_tables`: the chunk reads the
// call's tables; else it owns them in `ws` and its chain makes them.  *pos: their position list, for the extraction.
int build_pruned_derived(ssw_ctx* ctx, ssw_ctx::Lane& ws, const void* rgb, PixFmt fmt, size_t n, size_t w, size_t h, size_t k,
                         const uint32_t* idx, const PruneSetup& ps, uint32_t* info, bool call_tables, Chain& ch, const uint32_t** pos) {
    const size_t cap = ps.plan.cap_total, lines = n * h;
    const bool deep = plan_is_deep(ps.rows), level2 = plan_is_level2(ps.rows);
    ssw_ctx::Lane::Pruned v;
    SSW_TRY(ws.pruned_derived(deep ? 0 : dct_pair_operand_elems(n, w, h) * sizeof(double), n * h * cap * sizeof(float),
                              ps.rows.split ? split_scratch_elems(n, w, h) * sizeof(double) : 0, v));
    PrunedChunk q{ctx, RowInput::rgb(fmt, rgb), n, w, h, k, lines, idx, !call_tables, v.sp, {v.o[0], v.o[1], v.o[2], v.o[3]}, v.rows};
    SSW_TRY(lay_out_prune_tables(ctx, call_tables ? nullptr : &ws, ps, w, info, q.t));
    *pos = q.t.pos;
    // operand planes: by number in the split scratch, else the lane's buffers as the two- / three-level pre-passes fill them
    PairPlanes pp;
    pp.sp = pp.l2 = q.sp;
    pp.p8 = lines * dct_pair_split_kpad(w);
    pp.p16 = pp.l2_plane = lines * dct_pair_split_kpad(w / 2);
    for (unsigned c = 0; c < ps.plan.n_classes; ++c) {
        const PruneClassSrc& s = ps.src[c];
        q.t.c[c].x = s.lane_buf >= 0 ? q.o[s.lane_buf] : pp.plane(level2, s.p1);
        q.t.c[c].x2 = s.split ? pp.plane(level2, s.p2) : nullptr;
    }
    // (a single frame is 135 blocks of 16 lines for 256 CUs: the merged launches of the gathered route are 35 us faster there)
    std::array<DerivedFusedClass, 9> fca{};
    if (level2) for (unsigned c = 0; c < 9; ++c) fca[c] = q.t.fused(c < ps.plan.n_classes ? c : 0);
    if (level2 && plan_derived_fused(ps.rows, lines) && dct_pair_derived_fused_fits(ps.plan.n_classes, fca.data())) pruned_rows_fused(q, fca, ch);
    else pruned_rows_gathered(q, ch);
    return pruned_cols(ctx, ws, n, cap, h, ch);
}

// Prune -> look once -> redo: build_chunk(chunk, lane, chain, pruned) through the pipeline; where it pruned, ONE wait for the
// device to read the info blocks in ctx->shared.overflow (one per chunk, or one for the call), the counters, and every chunk whose
// block has the overflow flag set -- its columns did not fit the compact plane -- again on lane 0 with the full transform.
typedef std::function<int(size_t, ssw_ctx::Lane&, Chain&, bool)> PrunedChunkBuilder;
int run_pruned_pipeline(ssw_ctx* ctx, size_t n_chunks, const PruneSetup& ps, bool info_per_chunk, const PrunedChunkBuilder& build_chunk) {
    SSW_TRY(run_pipeline(ctx, n_chunks, [&](size_t ci, ssw_ctx::Lane& ws, Chain& ch) { return build_chunk(ci, ws, ch, ps.on); }));
    if (!ps.on) return SSW_OK;
    std::vector<uint32_t> info((info_per_chunk ? n_chunks : 1) * SSW_PRUNE_INFO);
    SSW_HIP_CHECK(hipMemcpyAsync(info.data(), ctx->shared.overflow.p, info.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    SSW_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    for (size_t ci = 0; ci < n_chunks; ++ci) {
        const uint32_t* block = info.data() + (info_per_chunk ? ci : 0) * SSW_PRUNE_INFO;
        ctx->pruned_chunks++;
        if (info_per_chunk || ci == 0)
            for (unsigned q = 0; q < ps.plan.n_classes; ++q) ctx->pruned_columns += block[1 + q];
        if (block[0] == 0) continue;
        ctx->redone_chunks++;
        Chain ch;
        SSW_TRY(build_chunk(ci, ctx->lane[0], ch, false));
        SSW_TRY(run_serial(ch, ctx->stream));
    }
    return SSW_OK;
}

// ---- base-reader pruning (base_prune.hip): who takes it, and its workspace -----------------------------------
// The terms of shape, alignment and plan: whole tiles and at least two, rows no shorter than columns, an ordering with a key
// bound, RGB frames the fused pre-pass reads, and the fused forward transform for `n` frames per chunk.  The CALL-level terms
// are not here: batch extract adds ctx->prune, the tuning entry base_prune and k <= select_max_k() (its masked selection) --
// switches between two ways to the same values; the debug entry ssw_debug_base_prune_bound shows what the decide kernel
// would compare for a shape, whether or not a call would currently take the path, so it applies none of them (its own k
// checks are those of its arguments).
bool base_prune_shape_ok(const ssw_ctx* ctx, const ssw_config& c, size_t n, size_t w, size_t h, const void* rgb, PixFmt fmt, const float* y, const float* tmp) {
    const bool f64 = c.precision == SSW_PRECISION_F64;
    if (!f64 || w % SSW_BASE_PRUNE_TILE != 0 || w / SSW_BASE_PRUNE_TILE < 2 || w < h || !(base_prune_gain(w, h, c.ordering) > 0.0f)) return false;
    if (!can_fuse_rgb(ctx, f64, w, h, y, tmp, rgb, fmt)) return false;
    const PlanInput in{SSW_DCT2, c.precision, n, w, h, 0, false, true, plan_settings(ctx)};
    return n <= plan_frame_limit(plan_settings(ctx), f64, w, h) && plan_pass(in, true, true).strategy == PassStrategy::FusedRows &&
           plan_pass(in, false, false).strategy == PassStrategy::FusedCols;
}
// energy [frames][W] f32 | need [frames][W / 128] u32 in the lane's buffer
int base_prune_workspace(ssw_ctx::Lane& ws, size_t frames, size_t w, BaseReaderArgs& a) {
    const size_t e_bytes = frames * w * sizeof(float);
    SSW_TRY(grow(ws.base_prune, e_bytes + frames * (w / SSW_BASE_PRUNE_TILE) * sizeof(unsigned)));
    a.energy = ws.base_prune.as<float>();
    a.need = (unsigned*)(ws.base_prune.as<char>() + e_bytes);
    return SSW_OK;
}
// What only the device knows of a pruned base reader's work is billed when the timers are resolved (flush_timers), from the
// context's counters: the second phase's share of the column launches and of the masked selection's reads (the computed tiles
// beyond every frame's tile 0, which the host billed), and the jobs of the gated tail row launches (base_energy.hip), counted
// by the launches themselves.  Each frame at its own shape's rate: the kernels add flop and bytes up as doubles; what was
// enqueued while the timers were off is passed over, like every other stage's work.
int base_prune_bill(ssw_ctx* ctx) {
    if (!ctx->shared.base_prune_stats.p) return SSW_OK;
    BasePruneCounters c;
    SSW_HIP_CHECK(hipMemcpy(&c, ctx->shared.base_prune_stats.p, sizeof(c), hipMemcpyDeviceToHost));
    const double now[5] = {c.col_flop, c.col_bytes, c.select_bytes, c.tail_flop, c.tail_bytes};
    double* billed = ctx->base_prune_billed;
    if (ctx->timing) {
        ctx->stage_work[SSW_STAGE_DCT_COL] += now[0] - billed[0];
        ctx->stage_bytes[SSW_STAGE_DCT_COL] += now[1] - billed[1];
        ctx->stage_work[SSW_STAGE_SELECT] += now[2] - billed[2];       // (an HBM-bound stage: its bytes are its work)
        ctx->stage_bytes[SSW_STAGE_SELECT] += now[2] - billed[2];
        ctx->stage_work[SSW_STAGE_DCT_ROW] += now[3] - billed[3];
        ctx->stage_bytes[SSW_STAGE_DCT_ROW] += now[4] - billed[4];
    }
    for (int i = 0; i < 5; ++i) billed[i] = now[i];
    return SSW_OK;
}

// extract (+ similarity against `marks`) of one chunk of batch extract: the derived values from full coefficient planes
// (pos null), or from the compact plane [n][h][cap] through the tables' position list
void push_extract_stage(Chain& ch, ssw_ctx* ctx, const ssw_config& c, const float* yb, const float* derived, const uint32_t* pos, size_t cap,
                        size_t n, size_t w, size_t h, const uint32_t* idx, size_t k, float* ext, const float* marks, float* sims) {
    ch.push_back({true, [=](hipStream_t st) -> int {
        if (k > 0) {
            StageTimer t(ctx, SSW_STAGE_EXTRACT, st);                           // :529-539
            if (pos) SSW_TRY(launch_extract_pruned(st, yb, derived, n, w, h, cap, pos, idx, k, c.method, c.alpha, ext));
            else SSW_TRY(launch_extract(st, yb, derived, n, w * h, idx, k, c.method, c.alpha, ext));
        }
        if (marks) {
            StageTimer t(ctx, SSW_STAGE_SIMILARITY, st);                        // :696-714
            SSW_TRY(launch_similarity(st, ext, marks, n, k, sims));
        }
        return SSW_OK;
    }});
}

}  // namespace

// ---- Writer::new + Writer::mark, batched ------------------------------------------------------------------
int batch_embed_impl(ssw_ctx* ctx, const ssw_config* cfg, const void* dev_rgb, PixFmt fmt_in, size_t n_frames, size_t w,
                     size_t h, const float* dev_marks, size_t k, void* dev_rgb_out, bool u8_out, float* dev_coef_out,
                     uint32_t* dev_indices_out) {
    if (!ctx || !dev_rgb || !dev_marks || !dev_rgb_out) return SSW_ERR_BAD_ARG;
    SSW_TRY(check_config(cfg));
    if (w == 0 || h == 0) return SSW_ERR_BAD_DIMS;
    const size_t plane = w * h;
    const size_t k_eff = std::min(k, plane - 1);                       // zip() truncation, :396: a longer mark is cut silently
    CtxGuard g(ctx);
    const size_t chunk = effective_chunk(ctx, w, h, n_frames);
    const size_t n_chunks = (n_frames + chunk - 1) / chunk;
    const ssw_config c = *cfg;
    const size_t in_px = 3 * pix_bytes(fmt_in), out_px = u8_out ? 3 : 3 * sizeof(float);
    auto build = [&](size_t ci, ssw_ctx::Lane& ws, Chain& ch) -> int {
        const size_t f0 = ci * chunk, n = std::min(chunk, n_frames - f0);
        ssw_ctx::Lane::WriterPlanes pl;
        SSW_TRY(ws.writer_planes(chunk * plane * sizeof(float), pl));
        SSW_TRY(grow(ws.idx, chunk * std::max<size_t>(k_eff, 1) * sizeof(uint32_t)));
        float *y = pl.y, *pi = pl.i, *pq = pl.q, *tmp = pl.scratch;
        const char* rgb = static_cast<const char*>(dev_rgb) + f0 * plane * in_px;
        char* out = static_cast<char*>(dev_rgb_out) + f0 * plane * out_px;
        uint32_t* idx = dev_indices_out ? dev_indices_out + f0 * k_eff : ws.idx.as<uint32_t>();
        float* coef_out = dev_coef_out ? dev_coef_out + f0 * plane : nullptr;
        const float* marks = dev_marks + f0 * k;
        SelectWorkspace* sel = &ws.sel;
        SSW_TRY(build_forward_from_rgb(ctx, ws, c.precision, rgb, fmt_in, n, w, h, y, pi, pq, tmp, ch));   // Writer::new :308-313
        ch.push_back({true, [=](hipStream_t st) -> int {
            if (coef_out) { SSW_HIP_CHECK(hipMemcpyAsync(coef_out, y, n * plane * sizeof(float), hipMemcpyDeviceToDevice, st)); untimed_work(ctx); }
            if (k_eff == 0) return SSW_OK;
            SSW_TRY(topk(ctx, st, *sel, y, n, w, h, c.ordering, k_eff, idx));                              // :314 (first k only)
            StageTimer t(ctx, SSW_STAGE_EMBED, st);                                                       // :356
            return launch_embed(st, y, n, plane, idx, k_eff, marks, nullptr, nullptr, 1, k_eff, k, c.method, c.alpha);
        }});
        Xform inv{SSW_DCT3, c.precision, n, w, h, y, tmp};                                                // :368-374
        inv.iq_i = pi; inv.iq_q = pq; inv.rgb_out = out; inv.rgb_out_u8 = u8_out;                        // + :377 in the last pass
        bool fused_rgb = false;
        SSW_TRY(build_transform(ctx, ws, inv, ch, &fused_rgb));
        if (fused_rgb) return SSW_OK;
        const double out_bytes = (double)n * plane * (12.0 + (u8_out ? 3.0 : 12.0));
        ch.push_back({true, [=](hipStream_t st) -> int {
            StageTimer t(ctx, SSW_STAGE_YIQ_TO_RGB, st, out_bytes);                                       // :377 (+ into_rgb8)
            if (u8_out) return launch_yiq_to_rgb8(st, y, pi, pq, n * plane, reinterpret_cast<uint8_t*>(out));
            return launch_yiq_to_rgb(st, y, pi, pq, n * plane, reinterpret_cast<float*>(out));
        }});
        return SSW_OK;
    };
    return run_pipeline(ctx, n_chunks, build);
}

// ---- Reader::base + Reader::derived + extract (+ Tester::similarity), batched --------------------------------
int batch_extract_impl(ssw_ctx* ctx, const ssw_config* cfg, const void* dev_base_rgb, const void* dev_derived_rgb, PixFmt fmt,
                       size_t n_frames, size_t w, size_t h, size_t k, float* dev_extracted, const float* dev_marks,
                       float* dev_sims) {
    if (!ctx || !dev_base_rgb || !dev_derived_rgb || !dev_extracted) return SSW_ERR_BAD_ARG;
    if ((dev_marks == nullptr) != (dev_sims == nullptr)) return SSW_ERR_BAD_ARG;
    SSW_TRY(check_config(cfg));
    if (w == 0 || h == 0) return SSW_ERR_BAD_DIMS;
    const size_t plane = w * h;
    if (k >= plane) return SSW_ERR_K_TOO_LARGE;                        // :553-555
    if (n_frames == 0) return SSW_OK;
    CtxGuard g(ctx);
    const size_t chunk = effective_chunk(ctx, w, h, n_frames);
    const size_t n_chunks = (n_frames + chunk - 1) / chunk;
    const ssw_config c = *cfg;
    const bool f64 = c.precision == SSW_PRECISION_F64;
    const size_t px_bytes = 3 * pix_bytes(fmt);
    // planes of lane 0 decide the (alignment-dependent) strategy for all lanes: hipMalloc'd, always 256-byte aligned
    // (lane 1 only when the call will run two lanes: three chunks or more)
    ssw_ctx::Lane::ReaderPlanes of_lane[ssw_ctx::MAX_LANES];
    for (int l = 0; l < (pipeline_uses_two_lanes(ctx, n_chunks) ? 2 : 1); ++l) SSW_TRY(ctx->lane[l].reader_planes(chunk * plane * sizeof(float), of_lane[l]));
    const float *y0 = of_lane[0].y, *tmp0 = of_lane[0].scratch;
    const PruneSetup ps = stream_capturing(ctx) ? PruneSetup() : make_prune_setup(ctx, f64, std::min(chunk, n_frames), w, h, k, y0, tmp0, dev_derived_rgb, fmt);
    if (ps.on) SSW_TRY(grow(ctx->shared.overflow, n_chunks * SSW_PRUNE_INFO * sizeof(uint32_t)));      // a block per chunk: every frame has its own list
    uint32_t* overflow = ctx->shared.overflow.as<uint32_t>();
    // Base-reader pruning (base_prune.hip): where the planner takes the fused forward transform for the chunks of this call
    // and the ordering has a key bound.  ssw_ctx_set_prune(0) and the tuning entry base_prune = 0 give the full transform.
    bool base_prune = ctx->prune && tuning(TUNE_BASE_PRUNE) != 0 && k > 0 && k <= select_max_k();
    for (size_t f0 = 0; base_prune && f0 < n_frames; f0 += chunk)        // (the last chunk may be shorter: another plan)
        base_prune = base_prune_shape_ok(ctx, c, std::min(chunk, n_frames - f0), w, h, dev_base_rgb, fmt, y0, tmp0);
    if (base_prune && !ctx->shared.base_prune_stats.p) {
        SSW_TRY(grow(ctx->shared.base_prune_stats, sizeof(BasePruneCounters)));
        SSW_HIP_CHECK(hipMemsetAsync(ctx->shared.base_prune_stats.p, 0, sizeof(BasePruneCounters), ctx->stream));
        untimed_work(ctx);
    }

    auto build_chunk = [&](size_t ci, ssw_ctx::Lane& ws, Chain& ch, bool pruned) -> int {
        const size_t f0 = ci * chunk, n = std::min(chunk, n_frames - f0);
        ssw_ctx::Lane::ReaderPlanes pl;
        SSW_TRY(ws.reader_planes(chunk * plane * sizeof(float), pl));
        SSW_TRY(grow(ws.idx, chunk * std::max<size_t>(k, 1) * sizeof(uint32_t)));
        float *yb = pl.y, *tmp = pl.scratch;
        uint32_t* idx = ws.idx.as<uint32_t>();
        const char* brgb = static_cast<const char*>(dev_base_rgb) + f0 * plane * px_bytes;
        const char* drgb = static_cast<const char*>(dev_derived_rgb) + f0 * plane * px_bytes;
        SelectWorkspace* sel = &ws.sel;
        // Reader::base (:474-480): only the Y plane is ever used by a reader
        const unsigned* mask = nullptr;         // set: the transform took the two-phase column pass, skipped tiles are stale
        if (base_prune) {
            BaseReaderArgs a;
            SSW_TRY(base_prune_workspace(ws, chunk, w, a));
            a.counters = ctx->shared.base_prune_stats.as<BasePruneCounters>();
            a.k = k; a.ordering = c.ordering;
            SSW_TRY(build_base_reader(ctx, ws, c.precision, brgb, fmt, n, w, h, yb, tmp, a, ch, &mask));
        } else {
            SSW_TRY(build_forward_from_rgb(ctx, ws, c.precision, brgb, fmt, n, w, h, yb, nullptr, nullptr, tmp, ch));
        }
        if (k > 0)
            ch.push_back({true, [=](hipStream_t st) -> int { return topk(ctx, st, *sel, yb, n, w, h, c.ordering, k, idx, mask); }});   // :493
        // Reader::derived: the compact plane of the columns the lists read, or (the un-pruned path and the redo) the full plane
        const float* derived = nullptr;
        const uint32_t* pos = nullptr;
        if (pruned) {
            SSW_TRY(build_pruned_derived(ctx, ws, drgb, fmt, n, w, h, k, idx, ps, overflow + ci * SSW_PRUNE_INFO, false, ch, &pos));
            derived = ws.compact.cols.as<float>();
        } else {
            float* full = nullptr;
            SSW_TRY(ws.derived_plane(chunk * plane * sizeof(float), &full));
            SSW_TRY(build_forward_from_rgb(ctx, ws, c.precision, drgb, fmt, n, w, h, full, nullptr, nullptr, tmp, ch));
            derived = full;
        }
        push_extract_stage(ch, ctx, c, yb, derived, pos, ps.plan.cap_total, n, w, h, idx, k, dev_extracted + f0 * k,
                           dev_marks ? dev_marks + f0 * k : nullptr, dev_sims ? dev_sims + f0 : nullptr);
        return SSW_OK;
    };
    return run_pruned_pipeline(ctx, n_chunks, ps, true, build_chunk);
}

// ssw_debug_base_prune_bound: what the decide kernel compares, for tests -- the chunk's forward transform as the batch
// path builds it (so the energies are the ones it would use), then G * E per natural column
int base_prune_bound_impl(ssw_ctx* ctx, const ssw_config* cfg, const float* dev_rgb, size_t n_frames, size_t w, size_t h, size_t k,
                          float* dev_bound) {
    const ssw_config c = *cfg;
    if (w == 0 || h == 0) return SSW_ERR_BAD_DIMS;
    if (n_frames == 0) return SSW_OK;
    const size_t plane = w * h;
    ssw_ctx::Lane& ws = ctx->lane[0];
    ssw_ctx::Lane::ReaderPlanes pl;
    SSW_TRY(ws.reader_planes(n_frames * plane * sizeof(float), pl));
    if (k == 0 || k >= plane || !base_prune_shape_ok(ctx, c, n_frames, w, h, dev_rgb, PixFmt::F32, pl.y, pl.scratch))
        return SSW_ERR_UNSUPPORTED;
    BaseReaderArgs a;
    SSW_TRY(base_prune_workspace(ws, n_frames, w, a));
    a.k = k; a.ordering = c.ordering;
    Chain ch;
    const unsigned* mask = nullptr;
    SSW_TRY(build_base_reader(ctx, ws, c.precision, dev_rgb, PixFmt::F32, n_frames, w, h, pl.y, pl.scratch, a, ch, &mask));
    SSW_TRY(run_serial(ch, ctx->stream));
    untimed_work(ctx);
    return launch_base_prune_bound(ctx->stream, a.energy, n_frames, w, h, c.ordering, dev_bound);
}

// ---- one base frame against many suspect frames (ssw_fingerprint_trace) -----------------------------------------
// Reader::base of the one original (:474-480, :493): plane and index list into buffers the CONTEXT owns -- every chunk on
// both lanes reads them.  On the context's stream, with lane 0's workspace (the suspects' pipeline starts behind it).
int trace_base(ssw_ctx* ctx, const ssw_config& c, const void* dev_base_rgb, PixFmt fmt, size_t w, size_t h, size_t k, const float** y,
               const uint32_t** idx) {
    const size_t plane = w * h;
    ssw_ctx::Lane& ws = ctx->lane[0];
    float* tmp = nullptr;
    SSW_TRY(grow(ctx->trace.base_plane, plane * sizeof(float)));
    SSW_TRY(grow(ctx->trace.base_idx, std::max<size_t>(k, 1) * sizeof(uint32_t)));
    SSW_TRY(ws.reader_scratch(plane * sizeof(float), &tmp));
    float* yb = ctx->trace.base_plane.as<float>();
    uint32_t* ib = ctx->trace.base_idx.as<uint32_t>();
    Chain ch;
    SSW_TRY(build_forward_from_rgb(ctx, ws, c.precision, dev_base_rgb, fmt, 1, w, h, yb, nullptr, nullptr, tmp, ch));
    SSW_TRY(run_serial(ch, ctx->stream));
    if (k > 0) SSW_TRY(topk(ctx, ctx->stream, ws.sel, yb, 1, w, h, c.ordering, k, ib));
    *y = yb;
    *idx = ib;
    return SSW_OK;
}

// base.extract(Reader::derived(suspect_s), k) for n_frames suspects (:529-561): the derived half of batch_extract_impl --
// same chunks, same lanes, same kernels up to the compact plane -- with the prune tables and gathered bases made once for
// the call (one list: the column set cannot grow with the batch, and there is one info block, so an overflow redoes every
// chunk) and the extraction that reads every base value once per slice of frames.
int trace_extract(ssw_ctx* ctx, const ssw_config& c, const float* yb, const uint32_t* idx, const void* dev_suspect_rgb, PixFmt fmt,
                  size_t n_frames, size_t w, size_t h, size_t k, float* dev_extracted) {
    if (n_frames == 0) return SSW_OK;
    const size_t plane = w * h;
    const size_t chunk = effective_chunk(ctx, w, h, n_frames);
    const size_t n_chunks = (n_frames + chunk - 1) / chunk;
    const size_t px_bytes = 3 * pix_bytes(fmt);
    const PruneSetup ps = stream_capturing(ctx) ? PruneSetup()
                          : make_prune_setup(ctx, c.precision == SSW_PRECISION_F64, std::min(chunk, n_frames), w, h, k, yb, yb, dev_suspect_rgb, fmt);
    if (ps.on) SSW_TRY(grow(ctx->shared.overflow, SSW_PRUNE_INFO * sizeof(uint32_t)));                 // one block: one list for the call
    uint32_t* info = ctx->shared.overflow.as<uint32_t>();
    if (ps.on) SSW_TRY(make_call_prune_tables(ctx, ps, w, k, idx, info));
    auto build_chunk = [&](size_t ci, ssw_ctx::Lane& ws, Chain& ch, bool pruned) -> int {
        const size_t f0 = ci * chunk, n = std::min(chunk, n_frames - f0);
        const char* srgb = static_cast<const char*>(dev_suspect_rgb) + f0 * plane * px_bytes;
        float* ext = dev_extracted + f0 * k;
        const uint32_t* pos = nullptr;                 // Reader::derived: the compact plane through the tables' position list, or the full plane
        float *full = nullptr, *tmp = nullptr;
        if (pruned) SSW_TRY(build_pruned_derived(ctx, ws, srgb, fmt, n, w, h, k, idx, ps, info, true, ch, &pos));
        else {
            SSW_TRY(ws.derived_plane(chunk * plane * sizeof(float), &full));
            SSW_TRY(ws.reader_scratch(chunk * plane * sizeof(float), &tmp));
            SSW_TRY(build_forward_from_rgb(ctx, ws, c.precision, srgb, fmt, n, w, h, full, nullptr, nullptr, tmp, ch));
        }
        const float* derived = pruned ? ws.compact.cols.as<float>() : full;
        const size_t cap = ps.plan.cap_total;
        ch.push_back({true, [=](hipStream_t st) -> int {
            StageTimer t(ctx, SSW_STAGE_EXTRACT, st);                               // :529-539
            if (pos) return launch_extract_shared_pruned(st, yb, derived, n, w, h, cap, pos, idx, k, c.method, c.alpha, ext);
            return launch_extract_shared(st, yb, derived, n, plane, idx, k, c.method, c.alpha, ext);
        }});
        return SSW_OK;
    };
    return run_pruned_pipeline(ctx, n_chunks, ps, false, build_chunk);
}

// ---- Reader::extract against ONE derived frame that has not been transformed yet (single-image handles) ------
// Reader::derived of the reference transforms the whole frame because it cannot know which coefficients will be
// read (:469-480); a derived handle therefore only uploads its frame, and the transform happens here, when the base
// reader's index list is known: the pruned transform of the batch path with n = 1 (same kernels, bit-identical
// values).  Enqueues on the context's stream: the k extracted values into dev_out, the overflow flag into
// dev_info[0] (non-zero: the columns did not fit, the caller must transform fully) -- enqueue-only, unlike
// run_pruned_pipeline: the caller reads the flag with the download of the result.  *applicable = false (nothing
// enqueued) when the shape or the settings do not take the pruned path.
int extract_single_pruned(ssw_ctx* ctx, int precision, const void* derived_rgb, PixFmt fmt, size_t w, size_t h, const float* base_y,
                          const uint32_t* idx, size_t k, int method, float alpha, float* dev_out, uint32_t** dev_info,
                          bool* applicable) {
    *applicable = false;
    const size_t plane = w * h;
    ssw_ctx::Lane& ws = ctx->lane[0];
    ssw_ctx::Lane::ReaderPlanes pl;
    SSW_TRY(ws.reader_planes(plane * sizeof(float), pl));
    const PruneSetup ps = make_prune_setup(ctx, precision == SSW_PRECISION_F64, 1, w, h, k, pl.y, pl.scratch, derived_rgb, fmt);
    if (!ps.on) return SSW_OK;
    SSW_TRY(grow(ctx->shared.overflow, SSW_PRUNE_INFO * sizeof(uint32_t)));
    uint32_t* info = ctx->shared.overflow.as<uint32_t>();
    Chain ch;
    const uint32_t* pos = nullptr;
    SSW_TRY(build_pruned_derived(ctx, ws, derived_rgb, fmt, 1, w, h, k, idx, ps, info, false, ch, &pos));
    SSW_TRY(run_serial(ch, ctx->stream));
    {
        StageTimer t(ctx, SSW_STAGE_EXTRACT, ctx->stream);
        SSW_TRY(launch_extract_pruned(ctx->stream, base_y, ws.compact.cols.as<float>(), 1, w, h, ps.plan.cap_total, pos, idx, k, method, alpha, dev_out));
    }
    *dev_info = info;
    *applicable = true;
    return SSW_OK;
}

}  // namespace host
}  // namespace ssw
