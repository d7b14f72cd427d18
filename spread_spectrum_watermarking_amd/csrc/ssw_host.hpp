// Host-side helpers shared by ssw_lib.hip (C ABI, handles) and ssw_pipeline.hip (transform chains and the
// two-lane batch pipelines).
#pragma once

#include <functional>
#include <vector>

#include "ssw_internal.hpp"

namespace ssw {
struct LadderTaps;               // resize_common.hpp
namespace host {

// v rounded up to a multiple of a
inline size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// Makes the context's GPU current for the duration of one ABI call and restores the caller's device
// afterwards (a host thread may drive several contexts, or torch on another GPU).
struct DeviceGuard {
    int prev = -1, dev;
    explicit DeviceGuard(int d) : dev(d) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) (void)hipSetDevice(dev);
    }
    ~DeviceGuard() {
        if (prev >= 0 && prev != dev) (void)hipSetDevice(prev);
    }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};

// DeviceGuard + "the context this thread is working for": dev_malloc() gives that context's pool of spare handle
// planes (up to SSW_PLANE_POOL_MB) back to the device and retries once before it reports out of memory.
struct CtxGuard {
    DeviceGuard dg;
    ssw_ctx* prev;
    explicit CtxGuard(ssw_ctx* ctx);
    ~CtxGuard();
};
// frees the spare planes of the context's pool; returns the bytes given back
size_t plane_pool_flush(ssw_ctx* ctx);

// Device allocation: a failing hipMalloc is reported as SSW_ERR_OUT_OF_MEMORY whatever code the runtime
// chose for it, and the runtime's sticky error is cleared so that the next call starts clean.  Before that the
// working context's plane pool is flushed and the allocation retried once.
int dev_malloc(void** p, size_t bytes);
#define SSW_ALLOC(pp, bytes) SSW_TRY(::ssw::host::dev_malloc((void**)(pp), (bytes)))
int grow(ssw_ctx::Buf& b, size_t bytes);
void release(ssw_ctx::Buf& b);
int grow_select(hipStream_t st, SelectWorkspace& s, size_t frames, size_t k);
void release_select(SelectWorkspace& s);

// transfer.hip: host buffers <-> device on `st`.  upload() returns once the caller's buffer may be reused
// (the data reaches the device in stream order), download() once the caller's buffer is complete.
int upload(ssw_ctx* ctx, void* dev_dst, const void* host_src, size_t bytes, hipStream_t st);
int download(ssw_ctx* ctx, void* host_dst, const void* dev_src, size_t bytes, hipStream_t st);
// The same for callers that keep every host buffer until they synchronise `st` themselves (the streaming entry
// points): a pinned buffer is only ENQUEUED (no wait); any other buffer takes the staged path above (upload: returns
// when staged; download: returns when complete).  *async_out: whether the transfer is still in flight on return.
int upload_nowait(ssw_ctx* ctx, void* dev_dst, const void* host_src, size_t bytes, hipStream_t st, bool* async_out);
int download_nowait(ssw_ctx* ctx, void* host_dst, const void* dev_src, size_t bytes, hipStream_t st, bool* async_out);
void transfer_destroy(ssw_ctx* ctx);
int transfer_set_threads(ssw_ctx* ctx, int threads);
int transfer_stats(ssw_ctx* ctx, double* out, bool reset);

// Stage timer: an event pair around a region on `st`, plus the work the region does (executed flop of the
// GEMM stages, algorithmic bytes of the HBM-bound ones) -- both only while timing is enabled.
struct StageTimer {
    ssw_ctx* ctx;
    int stage;
    hipStream_t st;
    hipEvent_t a = nullptr, b = nullptr;
    bool armed = false;
    int alias = -1;              // a second stage that this region IS (a pass that runs as its one "main" launch): same time, no events of its own
    StageTimer(ssw_ctx* c, int s, hipStream_t stream, double work = 0.0, int alias_stage = -1);
    ~StageTimer();
    // algorithmic HBM bytes of a GEMM stage (operands in, results and the inverse's E / T2 / A1 exchange out and in):
    // the HBM-bound stages' bytes ARE their work and are counted by the constructor
    void traffic(double bytes);
    StageTimer(const StageTimer&) = delete;
    StageTimer& operator=(const StageTimer&) = delete;
};
int flush_timers(ssw_ctx* ctx);
// Anything that is enqueued outside a StageTimer -- an event wait or record, an unbracketed launch or copy -- ends the sharing
// of the last timer's end event (ssw_pipeline.hip: timer_event): the next stage records its own start behind it and is not
// billed for it (a lane's hop to the other stream is a hipStreamWaitEvent: shared, it counted the dependency stall as stage time).
inline void untimed_work(ssw_ctx* ctx) { if (ctx) ctx->tail_fresh = false; }

// the cached basis `kind` of a length-n axis (made on first use); every kind but Dense is f64
int get_basis(ssw_ctx* ctx, size_t n, bool inverse, bool f64, BasisKind kind, const void** out);

bool valid_method(int m);
bool valid_ordering(int o);
bool valid_precision(int p);
int check_config(const ssw_config* cfg);
size_t effective_chunk(const ssw_ctx* ctx, size_t w, size_t h, size_t n_frames);

// ---- chains of stages -------------------------------------------------------------------------------
// A chain is the ordered list of device stages one chunk goes through.  Every stage is either HBM-bound
// (pre-passes, selection, colour conversion, O(k) kernels) or a group of basis-GEMM launches; the batch
// pipelines put the two kinds on different streams, everything else runs a chain on one stream.
struct Stage {
    bool hbm;
    std::function<int(hipStream_t)> run;
    int tag = 0;        // two-lane scheduling hints: 1 = the GEMM launches of a ROW pass, 2 = the RGB pre-pass that opens a forward transform
};
typedef std::vector<Stage> Chain;

// dct2d::dct2_2d on n contiguous planes, `data` in place, `tmp` same-size scratch; `ws` supplies the operand
// planes.  `rgb` (optional; rows-first forward transforms the fused pre-pass accepts, see can_fuse_rgb):
// the frames `data` would have been converted from -- the first pass reads them directly and `data` is
// only written by the last pass; iq_i / iq_q receive the I and Q planes (both or neither).
struct Xform {
    int type, precision;
    size_t n, w, h;
    float* data;
    float* tmp;
    const void* rgb = nullptr;
    PixFmt rgb_fmt = PixFmt::F32;   // sample format of `rgb`
    float* iq_i = nullptr;
    float* iq_q = nullptr;
    // inverse transforms (Writer::result): where the last pass may deliver RGB pixels instead of the Y plane
    // (iq_i / iq_q are then inputs); build_transform reports through `fused_rgb` whether it did
    void* rgb_out = nullptr;
    bool rgb_out_u8 = false;
    // intermediate plane of a deep forward transform in class-major column order (dct_pair_common.hpp): decided from
    // the frame's shape -- `full_h` when this Xform is a band of rows of a taller frame; `natural_order` forces the
    // natural order (the compact plane of the pruned transform has its own)
    size_t full_h = 0;
    bool natural_order = false;
};
int build_transform(ssw_ctx* ctx, ssw_ctx::Lane& ws, const Xform& x, Chain& ch, bool* fused_rgb = nullptr);
bool can_fuse_rgb(const ssw_ctx* ctx, bool f64, size_t w, size_t h, const float* y, const float* tmp, const void* rgb, PixFmt fmt);
// rgb -> Y (+ I, Q) -> forward transform of Y into `y` (Writer::new / Reader::new_impl), fused where possible
int build_forward_from_rgb(ssw_ctx* ctx, ssw_ctx::Lane& ws, int precision, const void* rgb, PixFmt fmt, size_t n, size_t w,
                           size_t h, float* y, float* i, float* q, float* tmp, Chain& ch);
// Reader::base of a batch extract (base_prune.hip): the same transform of Y only, with the column pass in two phases on the
// tiles that can hold one of the first k keys where the fused forward transform applies; *mask = `need` then, else null.
// One lane's buffers: energy [n][W] f32 | need [n][W / 128] u32; `counters`: the context's block, or null (nothing counted).
struct BaseReaderArgs {
    float* energy = nullptr;
    unsigned* need = nullptr;
    BasePruneCounters* counters = nullptr;
    size_t k = 0;
    int ordering = 0;
};
int build_base_reader(ssw_ctx* ctx, ssw_ctx::Lane& ws, int precision, const void* rgb, PixFmt fmt, size_t n, size_t w, size_t h, float* y,
                      float* tmp, const BaseReaderArgs& a, Chain& ch, const unsigned** mask);
// the same transform as bands + 1 chains: the row pass of a band of image rows (h / bands of them), and the column pass of the whole frame
bool can_split_forward_rows(const ssw_ctx* ctx, bool f64, size_t w, size_t h, size_t bands, const float* y, const float* tmp, const void* rgb, PixFmt fmt);
int build_forward_rows_band(ssw_ctx* ctx, ssw_ctx::Lane& ws, int precision, const void* rgb, PixFmt fmt, size_t w, size_t rows,
                            size_t frame_h, float* tmp, float* i, float* q, Chain& ch);
int build_forward_cols_after_rows(ssw_ctx* ctx, ssw_ctx::Lane& ws, int precision, size_t w, size_t h, float* tmp, float* y, Chain& ch);
int run_serial(Chain& ch, hipStream_t st);
// transform now, on the context's stream, with lane 0's workspace (handles, ssw_dct2d)
int dct2d_planes(ssw_ctx* ctx, int type, int precision, size_t n, size_t w, size_t h, float* data, float* tmp);

// first k entries of the reference's ordering for n planes (select.hip; full sort beyond its limit).  need: the tile mask of
// a pruned base reader (base_prune.hip), [n][w / SSW_BASE_PRUNE_TILE] -- tiles whose flag is 0 are not read
int topk(ssw_ctx* ctx, hipStream_t st, SelectWorkspace& sel, const float* coef, size_t n, size_t w, size_t h, int ordering,
         size_t k, uint32_t* idx, const unsigned* need = nullptr);

int batch_embed_impl(ssw_ctx* ctx, const ssw_config* cfg, const void* dev_rgb, PixFmt fmt_in, size_t n_frames, size_t w,
                     size_t h, const float* dev_marks, size_t k, void* dev_rgb_out, bool u8_out, float* dev_coef_out,
                     uint32_t* dev_indices_out);
int batch_extract_impl(ssw_ctx* ctx, const ssw_config* cfg, const void* dev_base_rgb, const void* dev_derived_rgb, PixFmt fmt,
                       size_t n_frames, size_t w, size_t h, size_t k, float* dev_extracted, const float* dev_marks,
                       float* dev_sims);

// ssw_debug_base_prune_bound: the row pass of n f32 base frames with the energy instances, then boundkey per natural column
int base_prune_bound_impl(ssw_ctx* ctx, const ssw_config* cfg, const float* dev_rgb, size_t n_frames, size_t w, size_t h, size_t k,
                          float* dev_bound);

// Tracing (ssw_fingerprint_trace; ssw_pipeline.hip).  trace_base: Reader::base of ONE frame + its first k indices into the
// context's buffers (*y, *idx), enqueued on the context's stream.  trace_extract: base.extract(Reader::derived(suspect_s), k)
// for n suspect frames against that plane and list -- chunks on two lanes, one prune plan for the call; looks at the
// overflow flag once when it pruned.  trace_score (ssw_lib.hip): similarity matrix + finish; sims may be null.
int trace_base(ssw_ctx* ctx, const ssw_config& c, const void* dev_base_rgb, PixFmt fmt, size_t w, size_t h, size_t k, const float** y,
               const uint32_t** idx);
int trace_extract(ssw_ctx* ctx, const ssw_config& c, const float* base_y, const uint32_t* base_idx, const void* dev_suspect_rgb, PixFmt fmt,
                  size_t n_frames, size_t w, size_t h, size_t k, float* dev_extracted);
int trace_check_args(const ssw_ctx* ctx, const ssw_config* cfg, size_t w, size_t h, size_t k, const void* marks, size_t n_marks,
                     const void* sims, const void* best, const void* best_sim, const void* n_exceed);
int trace_score(ssw_ctx* ctx, const float* dev_extracted, size_t n_suspects, const float* dev_marks, size_t n_marks, size_t k,
                float threshold, float* dev_sims, uint32_t* dev_best, float* dev_best_sim, uint32_t* dev_n_exceed);
// ssw_stream.hip: the host form -- suspects through the streaming ring, the base plane and list given (device).
// `placements` (normalised, one per suspect; null: every suspect is a frame [h][w][3]): host_suspects[s] is the suspect as it
// is and is restored on the device into its frame of the group, over `dev_base` (the original's pixels; may be null when no
// placement reads them)
int stream_trace_rgb8(ssw_ctx* ctx, const ssw_config& c, const float* base_y, const uint32_t* base_idx, const uint8_t* const* host_suspects,
                      size_t n_suspects, size_t w, size_t h, size_t k, const float* host_marks, size_t n_marks, float threshold,
                      float* host_extracted, float* host_sims, uint32_t* host_best, float* host_best_sim, uint32_t* host_n_exceed,
                      const ssw_placement* placements = nullptr, const uint8_t* dev_base = nullptr);

// Restoring attacked suspects before the trace (restore.hip; include/ssw.h: ssw_restore_rgb8).  restore_normalise: checks n
// placements against the frame and fills in pw = ph = 0 (SSW_ERR_BAD_ARG).  restore_prepare: caches every tap table the
// placements need -- the one step that may wait for the stream, so callers do it before their pipeline starts.
// restore_enqueue: the restore launches of n jobs (none of them restore_untouched) on the context's stream, one stage timer.
struct RestoreJob { const uint8_t* src; uint8_t* out; ssw_placement p; };      // device pointers; p normalised
bool restore_untouched(const ssw_placement& p, size_t w, size_t h);            // 3 channels, the frame's size, whole frame
bool restore_reads_base(const ssw_placement& p, size_t w, size_t h);           // the original's pixels are needed
int restore_normalise(const ssw_placement* pl, size_t n, size_t w, size_t h, std::vector<ssw_placement>* out);
int restore_prepare(ssw_ctx* ctx, const std::vector<ssw_placement>& pl);
int restore_enqueue(ssw_ctx* ctx, const uint8_t* dev_base, size_t w, size_t h, const RestoreJob* jobs, size_t n);
// locate.hip (include/ssw.h: ssw_locate_rgb8): pl normalised with x = y = 0 and prepared; host_res [n][2]: SAD, (y << 32) | x.
// Synchronises the context's stream.
// win (the refinement of ssw_locate_scaled_rgb8; null: every position): per entry the candidate positions x0..x1, y0..y1
// (inclusive, valid ones) it searches, and whether it is the same suspect at the same size as the entry before it
struct LocWindow { uint32_t x0, x1, y0, y1; bool share; };
// luma_planes (the refinement of ssw_locate_turned_rgb8): dev_suspects[i] is not a frame but its luma plane already,
// [ph][pw rounded up to 4] with zeros behind pw, read where it lies; pl[i] then has pw == w, ph == h.
int locate_impl(ssw_ctx* ctx, const uint8_t* dev_base, size_t w, size_t h, const void* const* dev_suspects,
                const std::vector<ssw_placement>& pl, uint64_t* host_res, const std::vector<LocWindow>* win = nullptr, bool luma_planes = false);
// locate.hip's planes of the original for the ladders (ssw_locate_scaled_rgb8, ssw_locate_turned_rgb8), enqueued on the context's
// stream: its luma plane (locate.luma) and the 2 x 2 phase planes of its 8 x 8 box means at every fourth position
// (locate.box_planes), rows of *qpitch bytes, *qrows of them, *plane_stride bytes apart.  w, h >= 8.
int locate_box8_planes(ssw_ctx* ctx, const uint8_t* dev_base, size_t w, size_t h, const uint8_t** planes, unsigned* qpitch, unsigned* qrows,
                       size_t* plane_stride);
// ... and one launch of box searches over them, m <= LOCATE_BATCH: search s is the template T [th][tpitch] of tw x th box means
// (tpitch % 4 == 0) at the nx x ny candidate positions (4 x, 4 y) into D [ny][nx]; keys[LOCATE_KEY_STRIDE s] (all ones before)
// receives (D << 32) | (y nx + x) of its smallest (D, y, x).  Timed as ssw_locate_scaled_rgb8 times its ladder.
constexpr unsigned LOCATE_BATCH = 32, LOCATE_KEY_STRIDE = 8;
struct BoxSearch { const uint8_t* T; uint32_t* D; uint32_t tpitch, tw, th, nx, ny; };
int locate_box_searches(ssw_ctx* ctx, const uint8_t* planes, unsigned qpitch, unsigned qrows, size_t plane_stride, const BoxSearch* it, unsigned m,
                        uint64_t* keys);
// locate.hip's scale ladder for locate_free.hip (ssw_locate_free_rgb8 starts from its answer): pl = w, h, channels of each suspect
// (checked), ranges [n][2] = wmin, wmax; one answer per suspect.  Waits for the stream twice.  upload_taps: every tap table of a
// call (resize_common.hpp: LadderTaps) into locate.taps with one copy on the context's stream; `taps` stays alive until the
// stream was waited for.
struct ScaledAnswer { uint32_t pw, ph, x, y; uint64_t sad; };
int locate_scaled_impl(ssw_ctx* ctx, const uint8_t* dev_base, size_t w, size_t h, const void* const* dev_suspects,
                       const std::vector<ssw_placement>& pl, const uint32_t* ranges, ScaledAnswer* out);
int upload_taps(ssw_ctx* ctx, const LadderTaps& taps, const uint32_t** dev);
// locate.hip's plane kernels for the angle search (angle.hip), enqueued on the context's stream: the luma planes of n frames
// [h][w][3] (rows of `pitch` bytes, pitch % 4 == 0), and of such planes the decimated 4 x 4 box means (h / 4 rows of `opitch` bytes)
int locate_luma_planes(ssw_ctx* ctx, const uint8_t* rgb, size_t n, size_t w, size_t h, uint8_t* out, size_t out_stride, unsigned pitch);
int locate_box4_planes(ssw_ctx* ctx, const uint8_t* luma, size_t luma_stride, unsigned lpitch, size_t n, size_t w, size_t h, uint8_t* out,
                       size_t out_stride, unsigned opitch);
// affine.hip's launches for the rotation search (angle.hip: ssw_rotate_search_attack_rgb8), enqueued on the context's stream: result i
// [h][w][3] at out + i * w * h * 3 is frame frames[i] of `in` (in_fb bytes apart) under m; fwd != null: the fused undo over `base`
// (BICUBIC).  affine_kept_enqueue: the pixels under the mask of the undoing (back, forward), added to *dev_count.
int affine_frames(ssw_ctx* ctx, const uint8_t* in, size_t in_fb, const uint32_t* frames, size_t n, size_t w, size_t h, const double* m,
                  const double* fwd, int filter, const uint8_t* fill, const uint8_t* base, uint8_t* out);
int affine_kept_enqueue(ssw_ctx* ctx, size_t w, size_t h, const double* back, const double* forward, unsigned long long* dev_count);
// ssw_lib.hip: the cached CatmullRom tap table (in_len -> out_len) of the context
int get_taps(ssw_ctx* ctx, size_t in_len, size_t out_len, DeviceTaps* out);

// fingerprint.hip: n_copies copies of one image, each Writer::result of `coef` with its own single mark embedded at `idx`
// (marks [n_copies][mark_stride]); enqueued on the context's stream; t32: an f32 plane of scratch
int fingerprint_copies(ssw_ctx* ctx, const ssw_config& c, const float* coef, const uint32_t* idx, size_t k_eff, const float* iq_i,
                       const float* iq_q, size_t w, size_t h, const float* marks, size_t mark_stride, size_t n_copies, void* out,
                       bool u8_out, float* t32);

// Reader::extract with a derived frame that is still RGB on the device (single-image handles): pruned transform +
// extraction enqueued on the context's stream; see ssw_pipeline.hip
int extract_single_pruned(ssw_ctx* ctx, int precision, const void* derived_rgb, PixFmt fmt, size_t w, size_t h, const float* base_y,
                          const uint32_t* idx, size_t k, int method, float alpha, float* dev_out, uint32_t** dev_info,
                          bool* applicable);

}  // namespace host
}  // namespace ssw
