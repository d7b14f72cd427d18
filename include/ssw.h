/*
 * ssw.h -- C ABI of the MI355X-native spread-spectrum watermarking hot path.
 *
 * Drop-in boundary for the `yiq -> dct2d -> ordering/top-k -> embed | extract ->
 * similarity` path of iwanders/spread_spectrum_watermarking.  The reference has
 * no FFI of its own (it is a pure-Rust crate); each entry point below replaces
 * the *body* of the reference function it cites (file:line relative to the
 * reference tree), and INTEGRATION.md shows the Rust `-sys` binding a maintainer
 * would add.  Plain pointers and sizes only; no exceptions or aborts cross this
 * boundary -- every call returns an ssw_status.
 *
 * Threading: a context is bound to one GPU and must be used by one host thread
 * at a time (like the reference's `!Send` Writer/Reader).  Multi-GPU = one
 * context (and one process or thread) per GPU; frames are independent so there
 * is no collective anywhere.
 *
 * Memory: "host" pointers are ordinary CPU memory; "dev" pointers are HIP device
 * memory on the context's GPU (e.g. from ssw_dev_alloc or a torch tensor's
 * data_ptr()).  Handles own their device planes; the caller owns all I/O buffers.
 */
#ifndef SSW_H
#define SSW_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum ssw_status {
    SSW_OK = 0,
    SSW_ERR_BAD_ARG = 1,          /* null pointer, unknown enum value                      */
    SSW_ERR_BAD_DIMS = 2,         /* w*h == 0 or data length != w*h   (src/dct2d.rs:90)     */
    SSW_ERR_LENGTH_MISMATCH = 3,  /* derived vs base length (src/algorithm.rs:550-552),
                                     similarity lengths (:697-700)                          */
    SSW_ERR_K_TOO_LARGE = 4,      /* extraction length >= coefficients (:553-555)           */
    SSW_ERR_NOT_BASE = 5,         /* derived reader used as base (:507, :530 unwrap)        */
    SSW_ERR_UNSUPPORTED = 6,      /* Custom(closure) variants cannot cross to the device    */
    SSW_ERR_CONSUMED = 7,         /* writer already consumed by mark()/result() (:355,:361) */
    SSW_ERR_HIP = 8,              /* HIP runtime error; see ssw_last_error()                */
    SSW_ERR_NO_DEVICE = 9,        /* no usable gfx950 device: there is NO CPU fallback      */
    SSW_ERR_OUT_OF_MEMORY = 10
} ssw_status;

/* OrderingMethod (src/algorithm.rs:143-152) */
typedef enum ssw_ordering {
    SSW_ORDER_ENERGY = 0,
    SSW_ORDER_ENERGY_ORTHOGONAL = 1,
    SSW_ORDER_LEGACY = 2,
    SSW_ORDER_CUSTOM = 3          /* -> SSW_ERR_UNSUPPORTED */
} ssw_ordering;

/* Insertion / Extraction (src/algorithm.rs:68-77, :115-124) */
typedef enum ssw_method {
    SSW_OPTION1 = 1,
    SSW_OPTION2 = 2,
    SSW_OPTION3 = 3,
    SSW_METHOD_CUSTOM = 4         /* -> SSW_ERR_UNSUPPORTED */
} ssw_method;

/* dct2d::Type (src/dct2d.rs:71-79) */
typedef enum ssw_dct_type {
    SSW_DCT2 = 0,
    SSW_DCT2_ORTHOGONAL = 1,
    SSW_DCT3 = 2
} ssw_dct_type;

/* Arithmetic of the DCT basis GEMMs (no counterpart in the reference, which
   delegates to rustdct's f32 FFT kernels). */
typedef enum ssw_precision {
    SSW_PRECISION_F32 = 0,        /* v_mfma_f32_32x32x2_f32: f32 fma chains of the dense GEMMs (no folding).
                                     NOT a parity path: extracted marks within 1e-4 in the median, 5e-3
                                     worst case; the slower precision wherever f64 folds */
    SSW_PRECISION_F64 = 1         /* DEFAULT.  v_mfma_f64_16x16x4_f64, f64 basis, result rounded
                                     once to f32: the correctly rounded ("canonical") transform,
                                     bit-identical extraction against the CPU restatement   */
} ssw_precision;

/* WriteConfig / ReadConfig (src/algorithm.rs:99-140).  ssw_config_default() is
   Option2(0.1) + Energy like the reference's Default impls (:104-111, :132-139), with the
   canonical (f64) transform precision. */
typedef struct ssw_config {
    int32_t ordering;             /* ssw_ordering  */
    int32_t method;               /* ssw_method    */
    float alpha;
    int32_t precision;            /* ssw_precision */
} ssw_config;

typedef struct ssw_ctx ssw_ctx;
typedef struct ssw_writer ssw_writer;
typedef struct ssw_reader ssw_reader;

/* ---- library / context ---------------------------------------------------- */
const char* ssw_version(void);
/* Always 0; the library has one build.  (Kept for callers of the former diagnostic build, which returned 1.) */
int ssw_build_all_strategies(void);
/* Which strategy of the 2-D transform (src/dct2d.rs:83-219) a batch of n_frames frames of w x h takes in the canonical (f64)
   precision under the context's current settings, as flags -- introspection for bench.py, DESIGN.md and the tests; every
   strategy computes the same values.  The flags are read off the plan that builds the passes (csrc/dct_plan.hpp, for the
   first group of frames on aligned planes), so they describe what runs at every folding level and split setting:
     PAIR_F64     operand-ready f64 GEMMs (otherwise the dense kernels)
     ROWS_DEEP / COLS_DEEP       one pre-pass per pass writes the operands of all launches (split odd halves)
     ROWS_LEVEL2 / COLS_LEVEL2   every launch of the pass sums len/16 terms (eight launches per pass)
     CLASS_MAJOR  the plane (or operand lines) between the passes in class-major order inside tiles of 128 columns
     FUSED_COLS   r5: no f32 plane between the passes -- the row launches' epilogue writes the column operands (forward only) */
enum { SSW_PLAN_PAIR_F64 = 1, SSW_PLAN_ROWS_DEEP = 2, SSW_PLAN_COLS_DEEP = 4, SSW_PLAN_ROWS_LEVEL2 = 8, SSW_PLAN_COLS_LEVEL2 = 16,
       SSW_PLAN_CLASS_MAJOR = 32, SSW_PLAN_FUSED_COLS = 64 };
int ssw_ctx_transform_plan(ssw_ctx* ctx, size_t n_frames, size_t w, size_t h, int dct_type, uint32_t* flags);
const char* ssw_status_string(int status);
/* Text of the last failing HIP call on this thread (empty string if none). */
const char* ssw_last_error(void);
void ssw_config_default(ssw_config* cfg);

/* One context per GPU.  Fails with SSW_ERR_NO_DEVICE when no HIP device is
   present -- the library never computes on the CPU. */
int ssw_ctx_create(int device_id, ssw_ctx** out);
int ssw_ctx_destroy(ssw_ctx* ctx);
int ssw_ctx_synchronize(ssw_ctx* ctx);
/* Stream contract.  Every entry point that takes "dev" pointers (ssw_rgb_to_yiq ... ssw_batch_*,
   ssw_resize_rgb8, ssw_synth_frames) only ENQUEUES work on the context's stream and returns; by default
   that is a private hipStreamNonBlocking stream, which is ordered neither against the null stream nor
   against e.g. torch's current stream.  The caller must therefore
     (1) make sure its inputs are complete before the call -- synchronise its producer, or hand the
         library an event to wait for (ssw_ctx_wait_event), or put the library on its own stream
         (ssw_ctx_set_stream);
     (2) treat outputs as valid only after ssw_ctx_synchronize(), or after an event recorded with
         ssw_ctx_record_event() has completed, or in later work on the stream given to ssw_ctx_set_stream.
   Entry points that take HOST buffers (the Writer / Reader / Tester handles, ssw_copy_*) return when the
   caller's buffers are theirs again: inputs have been read (staged or DMA'd), outputs are complete.  The
   device work a handle constructor started may still be running -- it is ordered before every later call
   on the same context, and a failure of it is reported by the next call that waits for the device.
   Calls change the calling thread's current HIP device only for their duration.
   One exception to "only enqueues": ssw_batch_extract* with pruning on (the default) waits once for the
   device at its end (see ssw_ctx_set_prune); while the context's stream is being captured into a graph it
   takes the full transform instead and does not wait. */
/* hipStream_t the context currently enqueues on, as an opaque pointer. */
void* ssw_ctx_stream(ssw_ctx* ctx);
/* Enqueue on the caller's hipStream_t from now on (NULL: back to the private stream).  Synchronises the
   stream used so far.  The stream must belong to the context's GPU and outlive its use here. */
int ssw_ctx_set_stream(ssw_ctx* ctx, void* hip_stream);
/* hipStreamWaitEvent / hipEventRecord on the context's stream with the caller's hipEvent_t: chain the
   library behind a producer, or a consumer behind the library, without a host synchronisation. */
int ssw_ctx_wait_event(ssw_ctx* ctx, void* hip_event);
int ssw_ctx_record_event(ssw_ctx* ctx, void* hip_event);
/* Frames processed per internal pass of the batch entry points (bounds the workspace: up to 44 bytes per
   pixel of a pass in the default GEMM strategy, per lane -- four f32 planes, row and column operand planes side
   by side since the fused forward transform, the inverse's A1 / T2 / E; see ssw_ctx_set_overlap).  0 = automatic, the
   default: about 2^30 pixels per pass (128 4K frames, 514 full-HD frames, 32 8K frames; up to 47 GB of
   workspace per lane): sized for the 288 GB of an MI355X, where longer GEMM launches amortise their tails
   (2^28 pixels cost 2.8 % at 4K, 1.8 % at full HD).  The automatic size never asks for more than half of what
   the device can give at the time of the call (free memory + what the context already holds): a smaller device
   or a co-tenant gets smaller passes, not SSW_ERR_OUT_OF_MEMORY. */
int ssw_ctx_set_chunk_frames(ssw_ctx* ctx, size_t frames);
/* Frames per pass a batch call over n_frames frames of w x h would use with the current setting. */
size_t ssw_ctx_pass_frames(ssw_ctx* ctx, size_t n_frames, size_t w, size_t h);

/* Batch pipelines (ssw_batch_*): two chunks in flight, each with its own workspace -- the HBM-bound stages
   of one (operand pre-passes, selection, colour conversion) run on a second internal stream while the
   basis GEMMs of the other run on the context's stream; the context's stream is ordered after all of it
   when the call returns.  Default on, used from two passes per call upwards (2 x 36 B/px of workspace
   then); 0 = one chunk at a time on one stream
   (what the per-kernel timings of bench.py's roofline leg use).  Results are bit-identical either way. */
int ssw_ctx_set_overlap(ssw_ctx* ctx, int enable);
/* ssw_batch_extract*: transform the derived frames only where Reader::extract reads them
   (src/algorithm.rs:556-561: k coefficients) -- the row pass for the frequency columns that occur in a
   chunk's index lists, the column pass on that compact plane; same operands, basis rows, kernel and
   summation order as the full transform, so the extracted values are bit-identical.  Falls back to the
   full transform per chunk when the columns do not fit 8 sqrt(k) slots, and altogether when that exceeds
   W/4 or the shape does not take the default GEMM strategy.  Default on; the call then waits once, at
   its end, for the device.  Handles (Reader::derived exposes coefficients()) always transform fully. */
int ssw_ctx_set_prune(ssw_ctx* ctx, int enable);
/* stats[0] chunks that took the pruned path, [1] of those redone with the full transform, [2] frequency
   columns actually needed (sum over chunks); since the last ssw_ctx_reset_timing. */
int ssw_ctx_get_prune_stats(ssw_ctx* ctx, uint64_t* stats);
/* Base-reader pruning of ssw_batch_extract* (on with ssw_ctx_set_prune and the tuning entry "base_prune", both default
   on; f64, Energy / EnergyOrthogonal, shapes whose forward transform is the fused one): the base frame's column pass runs
   on the 128-column tiles that can hold one of the first k keys -- tile 0, then the tiles whose per-column energy bound
   reaches the k-th key of tile 0 -- and the selection reads those tiles only; outputs are bit-identical to the full transform.
   stats[0] column tiles of the base frames, [1] of those computed, [2] frames whose second phase computed a tile; counted
   on the device since the last ssw_ctx_reset_timing.  Synchronises. */
int ssw_ctx_get_base_prune_stats(ssw_ctx* ctx, uint64_t* stats);
/* ... with the tuning entry "base_energy_lowp" (default on; rows of more than 1024 columns): the exact row launches compute
   the first 64-pair tile column of every launch class only, a low-precision kernel bounds the energies of the other columns
   from above, and the exact launches of those tile columns run after the decision, per frame, where a needed column tile
   reads them.  *jobs: the (frame, class, tail tile column) jobs that ran, counted on the device since the last
   ssw_ctx_reset_timing.  Synchronises. */
int ssw_ctx_get_base_prune_tail_jobs(ssw_ctx* ctx, uint64_t* jobs);
/* Diagnostic: the key bound of every frequency column of n f32 base frames, as the pruning of ssw_batch_extract forms it
   for mark length k (row pass only): dev_bound [n][w], natural column order.  SSW_ERR_UNSUPPORTED where that path does not
   apply to the shape / configuration.  Enqueues on the context's stream. */
int ssw_debug_base_prune_bound(ssw_ctx* ctx, const ssw_config* cfg, const float* dev_rgb, size_t n_frames, size_t w, size_t h,
                               size_t k, float* dev_bound);
/* Diagnostic: the top-k selection under a tile mask, as the pruned base reader runs it.  dev_need [n][w / 128] (u32; null: no
   mask): a 128-column tile whose flag is 0 is never read and its elements count as +0.0f.  cand_cap: candidate slots per
   frame (0: the default; fewer than k sends every frame through the exact whole-plane select).  dev_indices [n][k].
   Enqueues on the context's stream. */
int ssw_debug_select_masked(ssw_ctx* ctx, const float* dev_coef, size_t n_frames, size_t w, size_t h, int ordering, size_t k,
                            const uint32_t* dev_need, size_t cand_cap, uint32_t* dev_indices);
/* Top-k selection (the first k entries of the ordering of src/algorithm.rs:200-280): stats[0] frames selected, [1] of
   those whose sampled threshold left fewer than k or more than the candidate buffer's survivors, so that the finish ran
   the exact select over the whole plane (same result, one CU sorting the plane: a latency cliff; massive ties and
   constant planes take it by design, images should not); since the last ssw_ctx_reset_timing.  Synchronises.
   stats[0] is counted when a call enqueues its selection (replays of a captured graph are not counted), stats[1] on
   the device. */
int ssw_ctx_get_select_stats(ssw_ctx* ctx, uint64_t* stats);

/* Even/odd folding of the basis GEMMs (fewer multiply-adds for the same transform, exact in f64) where the frame shape
   allows (W % 8 == 0 / H % 8 == 0).  Folding runs in SSW_PRECISION_F64 only.  Strategy levels:
     0  dense GEMMs
     1  dense GEMMs (the in-kernel folding of round 1 was superseded by level 3 and removed)
     2  same as 1
     3  "operand-ready" GEMMs -- HBM-bound pre-passes write the folded operands once per pass as
        k-blocked f64 planes and the MFMA loop issues no VALU instruction
        (csrc/dct_pair_f64.hip, dct_pair_prep.hip); one level
     4  level 3 with the even half folded once more on row passes with W % 16 == 0 and column
        passes with H % 8 == 0 (3/8 of the dense MACs on that axis)
     5  default.  Level 4 plus a third folding level on forward row passes of at least 3072 columns
        (a multiple of 32): 11/32 of the dense MACs there
     6  level 5 without the size threshold (shorter rows lose more to the extra small launches than
        they save; for tests)
   All levels produce the same f64-accurate result rounded once to f32 (tests/test_gpu_parity.py).  Levels 1 / 2, and
   every level in SSW_PRECISION_F32, run the dense GEMMs. */
#define SSW_DCT_FOLDING_DEFAULT 5
int ssw_ctx_set_dct_folding(ssw_ctx* ctx, int level);
/* f64 precision, folding level 4 and up: the odd half of a folded transform (a DCT-IV of half the length, the one part
   that does not fold) is computed as a cosine and a sine transform of a quarter of the length each, after one plane
   rotation of its input pairs -- X[2j] = A[j] + B[j], X[2j-1] = A[j] - B[j] with a[n] = d[n] cos psi_n + d[M-1-n] sin psi_n,
   b[n] = d[M-1-n] cos psi_n - d[n] sin psi_n, psi_n = pi (2n+1) / (4M) -- and both of those fold once more: a quarter of
   the odd half's multiply-adds.  On axes whose length allows it (rows % 64 == 0 / columns % 16 == 0 forward, rows % 128 ==
   0 / columns % 16 == 0 inverse) one pre-pass applies this to the odd halves of two levels ("deep"), otherwise
   (length % 8 == 0) to the first.  The rotation is the one inexact step ahead of the f64 MFMA sums (relative error
   2^-52 of the operand); everything else stays an exact fold.  Results: the same f64-accurate transform rounded
   once to f32 -- equal to the unsplit GEMMs' output except where that rounding was within ~1e-9 ulp of a tie
   (tests/test_gpu_parity.py::test_odd_split_matches_exact_operands).  Default on; 0 = every operand an exact sum
   (the round-2 arithmetic, 1.8x the multiply-adds). */
int ssw_ctx_set_odd_split(ssw_ctx* ctx, int enable);

/* Strategy thresholds and A/B switches of the transform, process-wide (csrc/tuning.hip).  They choose between kernels that
   compute the same values (the strategies of src/dct2d.rs:83-219's one transform), never between results; tests lower a
   threshold so that small shapes the oracle finishes in seconds take the kernels of the 4K path.  Names (default):
     efold_min (1280), efold_inv_min (1280), efold_cols_min (720)   shortest forward row / inverse row / column pass at level 2
     deep_min_rows (256), deep_min_cols (256)                       shortest pass that takes the deep pre-passes
     merge_max_lines (8192) passes of at most this many lines run a stage's launches as one
     bn32 (-1)             32-pair tiles for small single-class launches: -1 automatic, 0 / 1 forced
     band_split (1)        single-image handles: row pass of the top half beside the upload of the bottom half
     fuse_cols (1)         forward transform: the row GEMMs' epilogue writes the column operands (no f32 plane between the passes)
     upload_bands (3)      single-image handles: bands of rows a host frame is uploaded and row-transformed in (2 .. 4)
     speculate_k (1)       Reader::base queues its selection for the mark length of the context's last extraction
     prep_light (1)        level-2 RGB row pre-pass in the < 64-VGPR form that fits beside GEMM blocks (0: the register-resident kernel)
     lane_stagger (1)      two lanes: an RGB pre-pass waits for the other lane's row launches and runs beside its column launches
     derived_fused (1)     the derived frame's pruned row pass in one kernel (0: pre-pass + gathered launches)
     tile48 (1)            48-pair GEMM tiles for classes whose 64-pair tiling ends in a tile of <= 16 pairs (135 = 48 + 48 + 39)
   An entry never set reads its SSW_<NAME> environment variable at first use (the r4 behaviour), else the default.
   ssw_tuning_set takes effect for the calls that follow; workspaces and cached plans of existing contexts were sized
   under the old values, so change a value before creating the context that should see it (tests use a fresh context).
   ssw_tuning_reset(NULL) returns every entry to environment / default.  Unknown name: SSW_ERR_BAD_ARG.
   Switches removed after measuring no gain are unknown names, and their SSW_* variables are ignored. */
int ssw_tuning_set(const char* name, long long value);
int ssw_tuning_get(const char* name, long long* value);
int ssw_tuning_reset(const char* name);

/* Per-stage device timers (hipEvent pairs on the context's stream).  DCT_ROW / DCT_COL cover the
   GEMM launches of a pass; at folding levels 3 / 4 the pre-passes are timed separately (DCT_PREP). */
typedef enum ssw_stage {
    SSW_STAGE_RGB_TO_YIQ = 0,     /* rgb -> y,i,q (24 B/px) or rgb -> y (16 B/px)   */
    SSW_STAGE_DCT_ROW = 1,        /* basis GEMM along the width                     */
    SSW_STAGE_DCT_COL = 2,        /* basis GEMM along the height                    */
    SSW_STAGE_SELECT = 3,         /* top-k ordering (radix select + sort)           */
    SSW_STAGE_EMBED = 4,
    SSW_STAGE_EXTRACT = 5,
    SSW_STAGE_SIMILARITY = 6,
    SSW_STAGE_YIQ_TO_RGB = 7,
    SSW_STAGE_RESIZE = 8,         /* CatmullRom resize of the attack harness         */
    SSW_STAGE_CONVERT = 9,        /* u8 <-> f32 frame conversion                     */
    SSW_STAGE_DCT_PREP = 10,      /* f64 operand pre-passes of folding levels 3 / 4 (HBM-bound) */
    SSW_STAGE_DCT_ROW_MAIN = 11,  /* the largest GEMM launch of a row pass alone (nested in DCT_ROW) */
    SSW_STAGE_DCT_COL_MAIN = 12,  /* the largest GEMM launch of a column pass alone (nested in DCT_COL) */
    SSW_STAGE_LOCATE = 13,        /* ssw_locate_rgb8: luma / box passes, coarse search, top-8, rescoring (bytes)  */
    SSW_STAGE_LOCATE_COARSE = 14, /* the coarse SAD launches alone (nested in LOCATE); work = byte differences     */
    SSW_STAGE_COUNT = 15
} ssw_stage;
int ssw_ctx_enable_timing(ssw_ctx* ctx, int enable);
int ssw_ctx_reset_timing(ssw_ctx* ctx);
/* Synchronises, then returns accumulated milliseconds and launch counts per stage
   (arrays of SSW_STAGE_COUNT). */
int ssw_ctx_get_timing(ssw_ctx* ctx, double* ms, uint64_t* launches);
/* Work done inside the timed regions, per stage (array of SSW_STAGE_COUNT): executed floating-point
   operations for the GEMM stages (DCT_ROW, DCT_COL and their *_MAIN launches), algorithmic bytes
   (what the stage must read and write once) for the HBM-bound ones. */
int ssw_ctx_get_work(ssw_ctx* ctx, double* work);
/* Algorithmic HBM bytes moved inside the timed regions, per stage (array of SSW_STAGE_COUNT): for the HBM-bound stages
   the same figure as ssw_ctx_get_work; for the GEMM stages (DCT_ROW, DCT_COL) the operand planes read, the results
   written and what the dependent launches of an inverse pass exchange (A1 / T2 / E out and in, I and Q in and RGB out in
   the last pass of Writer::result, src/algorithm.rs:361-379) -- each byte once, bases not counted (cache-resident).
   bench.py's `roofline_step` is built from it. */
int ssw_ctx_get_traffic(ssw_ctx* ctx, double* bytes);

/* Device memory helpers for hosts without their own allocator. */
int ssw_dev_mem_info(ssw_ctx* ctx, size_t* free_bytes, size_t* total_bytes);
int ssw_dev_alloc(ssw_ctx* ctx, size_t bytes, void** dev_ptr);
int ssw_dev_free(ssw_ctx* ctx, void* dev_ptr);
int ssw_copy_to_dev(ssw_ctx* ctx, void* dev_dst, const void* host_src, size_t bytes);
int ssw_copy_to_host(ssw_ctx* ctx, void* host_dst, const void* dev_src, size_t bytes);

/* Host <-> device transfers of the host-buffer entry points.  A pinned host buffer (ssw_host_alloc,
   hipHostMalloc, hipHostRegister) is the DMA source / target itself; any other buffer goes through a ring
   of pinned staging buffers in the context, filled / drained by a few host threads while the DMA of the
   previous slice runs (csrc/transfer.hip).  The reference has no counterpart: its images never leave the
   CPU (`DynamicImage` in, `DynamicImage` out, src/algorithm.rs:295, :355). */
int ssw_host_alloc(ssw_ctx* ctx, size_t bytes, void** host_ptr);      /* pinned (page-locked) host memory */
int ssw_host_free(ssw_ctx* ctx, void* host_ptr);
/* Host threads (the caller's included) that copy between pageable buffers and the staging ring:
   0 = automatic (4, or half the cores if fewer; environment: SSW_COPY_THREADS), 1 = the caller's only. */
int ssw_ctx_set_copy_threads(ssw_ctx* ctx, int threads);
typedef enum ssw_transfer_stat {
    SSW_TRANSFER_H2D_BYTES = 0,       /* bytes uploaded by host-buffer entry points                  */
    SSW_TRANSFER_D2H_BYTES = 1,
    SSW_TRANSFER_H2D_SECONDS = 2,     /* host wall time inside uploads (staging copy + DMA issue)    */
    SSW_TRANSFER_D2H_SECONDS = 3,     /* host wall time inside downloads (incl. waiting for results) */
    SSW_TRANSFER_STAGED_BYTES = 4,    /* of the above, bytes that went through the staging ring      */
    SSW_TRANSFER_DIRECT_BYTES = 5,    /* ... and bytes DMA'd straight from / to pinned caller memory */
    SSW_TRANSFER_STAT_COUNT = 6
} ssw_transfer_stat;
/* Copies the counters (array of SSW_TRANSFER_STAT_COUNT doubles; may be NULL) and optionally zeroes them. */
int ssw_ctx_get_transfer_stats(ssw_ctx* ctx, double* stats, int reset);

/* ---- transforms (device-resident, batched) --------------------------------- */

/* From<&Rgb32FImage> for YIQ32FImage, src/yiq.rs:177-186.  rgb: [n][h][w][3] f32.
   dev_i / dev_q may both be NULL (readers never use them: algorithm.rs:476). */
int ssw_rgb_to_yiq(ssw_ctx* ctx, const float* dev_rgb, size_t n_frames, size_t w, size_t h,
                   float* dev_y, float* dev_i, float* dev_q);
/* From<&YIQ32FImage> for Rgb32FImage, src/yiq.rs:187-197 (clamps to [0,1]). */
int ssw_yiq_to_rgb(ssw_ctx* ctx, const float* dev_y, const float* dev_i, const float* dev_q,
                   size_t n_frames, size_t w, size_t h, float* dev_rgb);
/* dct2d::dct2_2d, src/dct2d.rs:83-219, in place on n_frames contiguous row-major
   planes.  Same pass order (larger dimension first), same f32 store between the
   passes, same scaling points. */
int ssw_dct2d(ssw_ctx* ctx, int dct_type, int precision, size_t n_frames, size_t w, size_t h,
              float* dev_planes);

/* ---- ordering (src/algorithm.rs:200-280) ----------------------------------- */
/* First k entries of obtain_indices_by_function (src/algorithm.rs:200-210) for each of
   n_frames coefficient planes: stable descending order, DC skipped, ties -> lower index first.
   dev_indices: [n_frames][k] u32.  k <= w*h-1. */
int ssw_topk_indices(ssw_ctx* ctx, const float* dev_coef, size_t n_frames, size_t w, size_t h,
                     int ordering, size_t k, uint32_t* dev_indices);

/* ---- embed / extract / similarity on device-resident coefficient planes ---- */
/* Writer::embed_watermark, src/algorithm.rs:382-410.  marks: [n_frames][n_marks][k]
   f32 (every mark of length k); indices [n_frames][k]. */
int ssw_embed_coefficients(ssw_ctx* ctx, float* dev_coef, size_t n_frames, size_t plane_len,
                           const uint32_t* dev_indices, size_t k, int method, float alpha,
                           const float* dev_marks, size_t n_marks);
/* Reader::extract_watermark, src/algorithm.rs:543-562.  out: [n_frames][k]. */
int ssw_extract_coefficients(ssw_ctx* ctx, const float* dev_base, const float* dev_derived,
                             size_t n_frames, size_t plane_len, const uint32_t* dev_indices,
                             size_t k, int method, float alpha, float* dev_out);
/* Tester::similarity, src/algorithm.rs:696-714, n_pairs independent (extracted,
   mark) pairs of length k; sequential f32 accumulation order preserved. */
int ssw_similarity_batch(ssw_ctx* ctx, const float* dev_extracted, const float* dev_marks,
                         size_t n_pairs, size_t k, float* dev_sims);

/* One-extraction-many-marks testing (README.md:62; the CLI's loop over stored marks,
   examples/main.rs:369-415): sims[b][j] = Tester::new(extracted[b]).similarity(marks[j]) for
   n_extracted extracted marks against a database of n_marks stored marks of length k, as an
   (n_extracted x k) . (k x n_marks) GEMM on the f32 matrix cores.  Numerators are MFMA fma chains
   instead of the reference's sequential f32 sums (src/algorithm.rs:702-711): equal to 1e-4
   relative, not bit for bit; denominators keep the reference's order.  dev_sims: [n_extracted][n_marks]. */
int ssw_similarity_matrix(ssw_ctx* ctx, const float* dev_extracted, size_t n_extracted, const float* dev_marks,
                          size_t n_marks, size_t k, float* dev_sims);

/* ---- whole path, batched & device-resident (the bench path) ---------------- */
/* Writer::new + Writer::mark for n_frames frames (algorithm.rs:295-316, :355-379):
   rgb -> yiq -> DCT2 -> top-k -> embed -> DCT3 -> rgb.  One mark of length k per
   frame: dev_marks [n_frames][k].  A mark longer than w*h-1 is cut at w*h-1 entries like the
   reference's zip() does (:396); the stride of dev_marks stays k.  Optional outputs (may be NULL):
   dev_coef_out [n_frames][h][w] = Writer::coefficient_image() before embedding,
   dev_indices_out [n_frames][min(k, w*h-1)]. */
int ssw_batch_embed(ssw_ctx* ctx, const ssw_config* cfg, const float* dev_rgb, size_t n_frames,
                    size_t w, size_t h, const float* dev_marks, size_t k, float* dev_rgb_out,
                    float* dev_coef_out, uint32_t* dev_indices_out);
/* Reader::base + Reader::derived + extract (+ Tester::similarity when dev_marks
   is given) for n_frames frame pairs (algorithm.rs:462-562, :696-714).
   dev_extracted [n_frames][k]; dev_sims [n_frames] (NULL allowed with dev_marks NULL). */
int ssw_batch_extract(ssw_ctx* ctx, const ssw_config* cfg, const float* dev_base_rgb,
                      const float* dev_derived_rgb, size_t n_frames, size_t w, size_t h, size_t k,
                      float* dev_extracted, const float* dev_marks, float* dev_sims);

/* ---- 8-bit frames and the resize attack (device-resident, batched) --------- */
/* Arithmetic of the third-party `image 0.24.3` crate, restated from its published behaviour
   (parity unpinned beyond the reference's similarity asserts; identical to the CPU oracle). */
/* `DynamicImage::into_rgb32f()` for 8-bit input (call sites src/algorithm.rs:308, :476): v / 255. */
int ssw_convert_rgb8_to_f32(ssw_ctx* ctx, const uint8_t* dev_in, size_t n_values, float* dev_out);
/* `DynamicImage::into_rgb8()` from Rgb32F (tests/single_simple.rs:28): round(clamp(v,0,1) * 255). */
int ssw_convert_f32_to_rgb8(ssw_ctx* ctx, const float* dev_in, size_t n_values, uint8_t* dev_out);
/* `image::imageops::resize(img, nw, nh, FilterType::CatmullRom)` (tests/attack_resize.rs:17-36) on
   n_frames RGB8 frames [h][w][3] -> [nh][nw][3]. */
int ssw_resize_rgb8(ssw_ctx* ctx, const uint8_t* dev_in, size_t n_frames, size_t w, size_t h, size_t nw,
                    size_t nh, uint8_t* dev_out);
/* ssw_batch_embed / ssw_batch_extract on 8-bit frames: the u8 -> f32 conversion is fused into the
   colour kernels (3 instead of 12 B/px at the boundary); the embedded frames come back quantised
   like `into_rgb8()`.  Same reference lines as the f32 forms. */
int ssw_batch_embed_rgb8(ssw_ctx* ctx, const ssw_config* cfg, const uint8_t* dev_rgb, size_t n_frames,
                         size_t w, size_t h, const float* dev_marks, size_t k, uint8_t* dev_rgb_out);
int ssw_batch_extract_rgb8(ssw_ctx* ctx, const ssw_config* cfg, const uint8_t* dev_base_rgb,
                           const uint8_t* dev_derived_rgb, size_t n_frames, size_t w, size_t h, size_t k,
                           float* dev_extracted, const float* dev_marks, float* dev_sims);

/* ---- fingerprinting: many individually marked copies of one image (device-resident) ---- */
/* For each of n_copies marks: Writer::new(image, cfg).mark(&[&mark_i]) (algorithm.rs:295-316, :355-379),
   i.e. the loop of examples/main.rs:266-278 once per recipient.  dev_rgb: ONE frame [h][w][3];
   dev_marks [n_copies][k]; dev_rgb_out [n_copies][h][w][3]; dev_indices_out optional [min(k, w*h-1)].
   The forward transform, the selection and the inverse of the unmarked plane are computed once; each copy is then a
   rank-R f64 update of the second inverse pass (R = distinct first-pass lines among the k indices) fused with the colour
   conversion (csrc/fingerprint.hip).  Same numerical contract as ssw_batch_embed: within its f64 parity bars of every
   single-mark Writer::mark, not bit-identical to it.  A copy does not depend on the other marks of the call or on its
   position among them.  Marks longer than w*h-1 are cut like ssw_batch_embed (the stride of dev_marks stays k);
   n_copies == 0 returns what ssw_batch_embed returns for no frames; SSW_PRECISION_F32 and the Custom variants:
   SSW_ERR_UNSUPPORTED.  Stream contract of ssw_batch_embed (enqueues only; graph-capturable); copies go in groups, so
   the workspace stays bounded (about 2 GiB) for any n_copies.  Timed as SSW_STAGE_EMBED / SSW_STAGE_YIQ_TO_RGB. */
int ssw_fingerprint_embed(ssw_ctx* ctx, const ssw_config* cfg, const float* dev_rgb, size_t w, size_t h,
                          const float* dev_marks, size_t n_copies, size_t k, float* dev_rgb_out,
                          uint32_t* dev_indices_out);
/* The same on 8-bit frames (algorithm.rs:295-316, :355-379 with into_rgb32f() / into_rgb8() of the caller,
   examples/main.rs:271-278): u8 in, copies quantised like into_rgb8(). */
int ssw_fingerprint_embed_rgb8(ssw_ctx* ctx, const ssw_config* cfg, const uint8_t* dev_rgb, size_t w, size_t h,
                               const float* dev_marks, size_t n_copies, size_t k, uint8_t* dev_rgb_out,
                               uint32_t* dev_indices_out);
/* Handle form: copies of what embed(&[&mark_i]) + result() (algorithm.rs:348-352, :361-379) would give on n clones of
   this writer, as it stands now (its current coefficients, the ordering Writer::new fixed, :314).  Does NOT consume or
   modify the writer.  host_marks [n_copies][k]; host_out [n_copies][h][w][3] f32 / u8 (into_rgb8).  A consumed writer:
   SSW_ERR_CONSUMED. */
int ssw_writer_mark_copies(ssw_writer* wr, const float* host_marks, size_t n_copies, size_t k, float* host_out);
int ssw_writer_mark_copies_rgb8(ssw_writer* wr, const float* host_marks, size_t n_copies, size_t k, uint8_t* host_out);

/* ---- tracing: ONE original against many suspect frames and many stored marks (device-resident) ---- */
/* The read side of fingerprinting.  Per suspect s exactly (algorithm.rs:462-562, :696-714; the `test` loop of
   examples/main.rs:369-415):
       base  = Reader::base(original, cfg)
       ext_s = base.extract(Reader::derived(suspect_s), k)
       sims[s][j] = Tester::new(ext_s).similarity(mark_j)
   dev_base_rgb: ONE frame [h][w][3]; dev_suspect_rgb [n_suspects][h][w][3]; dev_marks [n_marks][k] or NULL.
   The base frame is transformed and ranked once per call; the suspects go through the pruned derived transform of
   ssw_batch_extract in chunks on two lanes, with one prune plan for the whole call (one index list, so the column set
   stays at its single-frame size).  Outputs:
     dev_extracted [n_suspects][k]   bit-identical to ssw_batch_extract(_rgb8) with the base frame replicated n_suspects
                                     times (the same kernels produce the values)
     dev_sims [n_suspects][n_marks]  (may be NULL) bit-identical to ssw_similarity_matrix(dev_extracted, dev_marks): the f32
                                     MFMA GEMM, equal to the reference's sums to 1e-4 relative
     dev_best [n_suspects]           (may be NULL) index of the largest non-NaN entry of row s, the lowest index on ties;
                                     0xFFFFFFFF when the row has none, when n_marks == 0 and when k == 0
     dev_best_sim [n_suspects]       (may be NULL) the winner rescored in the reference's sequential f32 order: equal bit for
                                     bit to ssw_similarity_batch(ext_s, mark_best), i.e. Tester::similarity itself (:702-713);
                                     NaN where there is no winner
     dev_n_exceed [n_suspects]       (may be NULL) entries of row s with sim > threshold; NaN never exceeds
                                     (Similarity::exceeds_sigma, :677).  Two colluders show as 2 -- for an averaged forgery; see the
                                     strength report (ssw_collude_rgb8 below).
   NaN is a real case: a suspect identical to the original extracts all zeros and every similarity is 0 / sqrt(0).
   Status codes follow ssw_batch_extract: k >= w*h SSW_ERR_K_TOO_LARGE (:553-555); n_suspects == 0 SSW_OK; dev_marks ==
   NULL requires n_marks == 0 and every similarity output NULL (extraction only), anything else SSW_ERR_BAD_ARG; Custom
   variants SSW_ERR_UNSUPPORTED; SSW_PRECISION_F32 takes the dense path.  Stream contract of ssw_batch_extract: enqueues
   only, except for one look at the prune overflow flag; under stream capture or with ssw_ctx_set_prune(ctx, 0) the
   suspects take the full transform (bit-identical outputs, no host wait).  When the column set does not fit the compact
   plane every chunk is redone in full.  ssw_ctx_get_prune_stats: a call counts its chunks, and its column set once. */
int ssw_fingerprint_trace(ssw_ctx* ctx, const ssw_config* cfg, const float* dev_base_rgb, const float* dev_suspect_rgb,
                          size_t n_suspects, size_t w, size_t h, size_t k, const float* dev_marks, size_t n_marks,
                          float threshold, float* dev_extracted, float* dev_sims, uint32_t* dev_best, float* dev_best_sim,
                          uint32_t* dev_n_exceed);
/* The same on 8-bit frames (algorithm.rs:462-562, :696-714 with into_rgb32f() of the caller, examples/main.rs:383-415). */
int ssw_fingerprint_trace_rgb8(ssw_ctx* ctx, const ssw_config* cfg, const uint8_t* dev_base_rgb, const uint8_t* dev_suspect_rgb,
                               size_t n_suspects, size_t w, size_t h, size_t k, const float* dev_marks, size_t n_marks,
                               float threshold, float* dev_extracted, float* dev_sims, uint32_t* dev_best,
                               float* dev_best_sim, uint32_t* dev_n_exceed);
/* Host form (algorithm.rs:462-562, :696-714; examples/main.rs:369-415 as one call): 8-bit host images, one pointer per
   suspect; marks and every output are host buffers (outputs may be NULL as above; host_extracted may be NULL too).  The base
   is uploaded and transformed once; the suspects stream through the ring of ssw_batch_extract_host_rgb8 (upload of group
   g + 1 under the kernels of group g).  Returns when every buffer is the caller's again.  Bit-identical to the device form. */
int ssw_fingerprint_trace_host_rgb8(ssw_ctx* ctx, const ssw_config* cfg, const uint8_t* host_base,
                                    const uint8_t* const* host_suspects, size_t n_suspects, size_t w, size_t h, size_t k,
                                    const float* host_marks, size_t n_marks, float threshold, float* host_extracted,
                                    float* host_sims, uint32_t* host_best, float* host_best_sim, uint32_t* host_n_exceed);
/* Handle form of the host call (algorithm.rs:529-539, :696-714): `base` is a base reader (else SSW_ERR_NOT_BASE); its
   transformed plane and its index list are reused, nothing of the original crosses PCIe again.  The reader stays usable. */
int ssw_reader_trace_host_rgb8(ssw_reader* base, const uint8_t* const* host_suspects, size_t n_suspects, size_t k,
                               const float* host_marks, size_t n_marks, float threshold, float* host_extracted,
                               float* host_sims, uint32_t* host_best, float* host_best_sim, uint32_t* host_n_exceed);

/* ---- tracing attacked copies: resized and cropped suspects are restored on the device ---- */
/* A leaked copy is rarely pixel-aligned with the original.  The reference's two attack tests are the recipe: resize the
   suspect back to the original's size with CatmullRom (tests/attack_resize.rs:31-36), and "complement the attacked image
   with the original to fill in the blanks" with Pixel::blend (tests/attack_crop.rs:56-70); then extract as usual.
   A placement says what a suspect is and where it lies in the original's frame. */
typedef struct ssw_placement {
    uint32_t w, h, channels;   /* the suspect as it is: [h][w][channels] u8, channels 3 (RGB) or 4 (RGBA) */
    uint32_t x, y, pw, ph;     /* the rectangle of the original's frame it covers; pw = ph = 0: its own size w, h */
} ssw_placement;
/* restore(original O [h][w][3], suspect S, placement) for n suspects -> dev_out [n][h][w][3]
   (tests/attack_resize.rs:31-36, tests/attack_crop.rs:56-70):
     1. R = S when (pw, ph) == (S.w, S.h), else imageops::resize(S, pw, ph, CatmullRom): every channel, alpha included,
        filtered on its own with the same taps, clamped and rounded exactly as ssw_resize_rgb8 does (the two share
        csrc/resize_common.hpp);
     2. out = O outside the rectangle (x, y, pw, ph); inside it out = R for 3 channels and rgb(blend(opaque O, R)) for 4,
        blend = Rgba<u8>::blend of `image 0.24.3`: a == 0 gives O, a == 255 gives R, otherwise in f32, un-fused, in this order
            bg = O / 255, fg = R / 255, fa = a / 255, ba = 1;  af = ba + fa - ba * fa;
            out_c = ((fg_c * fa) + (bg_c * ba) * (1 - fa)) / af;  byte = 255 * out_c truncated toward zero.
   Third-party arithmetic restated from the crate's published behaviour, like the resize: parity unpinned (the reference's
   own test only exercises alpha 0 and 255); the formula above is the contract, and the result equals this recipe bit for bit.
   dev_suspects / placements: HOST arrays of n device pointers / n placements.  No alignment is assumed of any pointer,
   x, w * channels or the frame's w * 3.  A suspect with 3 channels, the frame's size and the whole-frame placement is
   copied, not touched by any restore launch.  Enqueues on the context's stream like ssw_resize_rgb8 (no host
   synchronisation, except the one that uploads a tap table the context has not cached yet); launch descriptors travel as
   kernel arguments, 32 suspects per launch.  SSW_ERR_BAD_ARG: a rectangle that leaves the frame, channels not 3 or 4, any
   zero size; n == 0: SSW_OK.  Timed as SSW_STAGE_RESIZE. */
int ssw_restore_rgb8(ssw_ctx* ctx, const uint8_t* dev_base_rgb, size_t w, size_t h, const void* const* dev_suspects,
                     const ssw_placement* placements, size_t n, uint8_t* dev_out);
/* ssw_fingerprint_trace_host_rgb8 on suspects that are restored first (tests/attack_resize.rs:31-36,
   tests/attack_crop.rs:56-70, then algorithm.rs:462-562, :696-714): host_suspects[s] is [placements[s].h][placements[s].w]
   [placements[s].channels] u8.  Equals ssw_fingerprint_trace_host_rgb8 run on the frames ssw_restore_rgb8 produces, bit for
   bit in all five outputs; results are in the order of host_suspects, whatever grouping happens inside.  A suspect with
   3 channels, the frame's size and the whole-frame placement is not touched by any restore launch: a call made only of
   such suspects gives today's trace, bit for bit.  Suspects of different sizes stream through the ring of
   ssw_batch_extract_host_rgb8 as they are (upload of group g + 1 under the kernels of group g; the raw slots are sized
   for the largest suspect of the call) and are restored into the group's frames on the device: the workspace stays
   bounded for any n_suspects.  Status codes: placements as ssw_restore_rgb8 (SSW_ERR_BAD_ARG); n_suspects == 0 SSW_OK;
   the rest as the trace forms (SSW_ERR_K_TOO_LARGE, SSW_ERR_UNSUPPORTED for Custom).  Restore launches are timed as
   SSW_STAGE_RESIZE. */
int ssw_fingerprint_trace_restored_host_rgb8(ssw_ctx* ctx, const ssw_config* cfg, const uint8_t* host_base, size_t w, size_t h,
                                             const uint8_t* const* host_suspects, const ssw_placement* placements,
                                             size_t n_suspects, size_t k, const float* host_marks, size_t n_marks,
                                             float threshold, float* host_extracted, float* host_sims, uint32_t* host_best,
                                             float* host_best_sim, uint32_t* host_n_exceed);
/* Handle form (algorithm.rs:529-539, :696-714 after tests/attack_resize.rs:31-36, tests/attack_crop.rs:56-70): `base` is a
   base reader (else SSW_ERR_NOT_BASE); host_base_rgb are the original's pixels [h][w][3] u8 again -- a reader keeps the
   plane and the list, not the image -- and may be NULL when no suspect needs them (every suspect 3 channels on the whole
   frame).  Equals ssw_reader_trace_host_rgb8 on the frames ssw_restore_rgb8 produces, bit for bit in all five outputs. */
int ssw_reader_trace_restored_host_rgb8(ssw_reader* base, const uint8_t* host_base_rgb, const uint8_t* const* host_suspects,
                                        const ssw_placement* placements, size_t n_suspects, size_t k, const float* host_marks,
                                        size_t n_marks, float threshold, float* host_extracted, float* host_sims,
                                        uint32_t* host_best, float* host_best_sim, uint32_t* host_n_exceed);

/* ---- locating a cut-out: where in the original does a suspect lie? ---- */
/* The placement of a cut-out is what ssw_restore_rgb8 needs and what the finder of a leaked copy does not know.  The
   reference's crop test knows its rectangle (tests/attack_crop.rs:56-70); this is the search for it: a translation only --
   no rotation, no unknown scale.  The size (pw, ph) the suspect had in the original's frame is its own (pw = ph = 0) or
   given by the caller.  x, y of each placement are OUTPUTS; w, h, channels, pw, ph are inputs.
   Definition, per suspect S [h][w][c] against the original O [H][W][3]; everything is an integer, no sum depends on its
   order, and the result equals the numpy restatement in tests/test_locate_cpu.py exactly in x, y and SAD:
     1. R = S when (pw, ph) == (w, h), else the CatmullRom resize of S to pw x ph with exactly the taps, clamping and
        rounding of ssw_restore_rgb8 / ssw_resize_rgb8 (csrc/resize_common.hpp).  An alpha channel is ignored by the search:
        a cut-out that is mostly transparent is not supported.
     2. Luma L(p) = (77 R + 150 G + 29 B + 128) >> 8.
     3. Candidate positions: 0 <= x <= W - pw, 0 <= y <= H - ph.
     4. Coarse factor f = 4 when min(pw, ph) >= 64, else 1.  f = 1: B = L_O, S_f = L_R.  f = 4: B(x, y) =
        (sum_{0<=i,j<4} L_O(x + i, y + j) + 8) >> 4, the box mean at EVERY pixel position (not decimated); S_f(i, j) is the
        same box of L_R at (4 i, 4 j) for i < pw / 4, j < ph / 4 (integer division).
     5. Coarse cost D(x, y) = sum_{i,j} |S_f(i, j) - B(x + f i, y + f j)| at every candidate position (u32: 255 pw ph / 16
        fits).  For an exact cut-out D is 0 at the true position whatever its phase.
     6. The 8 positions with the smallest (D, y, x) in lexicographic order (all of them when fewer exist).
     7. For each of those SAD(x, y) = sum |L_R(i, j) - L_O(x + i, y + j)| over all pw ph pixels; the answer is the position
        with the smallest (SAD, y, x), and host_sad[s] its SAD (64 bits: 255 W H exceeds 32 at 8K).
   Known limit: a cut-out of a featureless region is ambiguous (many positions cost almost the same); the answer is still
   the one this definition names.
   dev_suspects / placements: HOST arrays of n device pointers / n placements; host_sad: HOST array of n.  No alignment is
   assumed of any pointer.  The call synchronises: the answer is needed on the host.  Suspects run in groups of at most
   256 MiB of workspace (one suspect's own need -- 4 bytes per candidate position, about 5 per pixel of R -- if that is more),
   so the workspace is bounded for any n.  SSW_ERR_BAD_ARG: a rectangle larger than the frame, channels not 3 or 4, any zero
   size; SSW_ERR_UNSUPPORTED: a resize that has no LDS tile (as ssw_restore_rgb8), 2^32 or more candidate positions;
   n == 0: SSW_OK.  Timed as SSW_STAGE_LOCATE (the coarse search also as SSW_STAGE_LOCATE_COARSE; the resize of step 1 as
   SSW_STAGE_RESIZE). */
int ssw_locate_rgb8(ssw_ctx* ctx, const uint8_t* dev_base_rgb, size_t w, size_t h, const void* const* dev_suspects,
                    ssw_placement* placements, size_t n, uint64_t* host_sad);

/* ---- locating a cut-out whose scale is unknown: a scale ladder ---- */
/* ssw_locate_rgb8 wants the size the cut-out had in the original; the finder of a part of the picture that was also scaled
   for the web does not know it.  This is the search over scale as well: per suspect a range of widths wmin <= wmax the
   cut-out may have had in the original.  pw, ph, x, y of each placement are OUTPUTS; w, h, channels are inputs.
   Definition, per suspect S [sh][sw][c] against the original O [H][W][3]; everything is an integer, no sum depends on its
   order, and the result equals the numpy restatement in tests/test_locate_scale_cpu.py exactly in pw, ph, x, y and SAD.
   Lumas and the CatmullRom resize are those of steps 1 and 2 of ssw_locate_rgb8 above; the aspect ratio is kept:
   ph(pw) = max(1, (2 sh pw + sw) / (2 sw)) (integer division).
     Rungs.  pw_j = wmin + 8 j while <= wmax, plus wmax if it was not hit.  Rungs with pw_j > W or ph_j > H are dropped.
       SSW_ERR_BAD_ARG if none is left, if wmin > wmax, or if min(wmin, ph(wmin)) < 32.
     Ladder cost of rung j.  R_j = the resize of S to pw_j x ph_j.  T_j(i, k) = (sum of the 8 x 8 lumas of R_j at (8 i, 8 k)
       + 32) >> 6 for i < pw_j / 8, k < ph_j / 8.  B8(x, y) = the same box mean of L_O, taken at every x, y that is a multiple
       of 4 and where the box fits.  D_j(x, y) = sum_{i,k} |T_j(i, k) - B8(x + 8 i, y + 8 k)| at the candidate positions x, y
       that are multiples of 4 with x <= W - pw_j, y <= H - ph_j.  The rung's entry is its smallest (D, y, x), with
       n_j = (pw_j / 8)(ph_j / 8) samples.
     Kept rungs.  The 8 rungs with the smallest D_j / n_j, compared by D_a n_b against D_b n_a in 64 bits; ties go to the
       smaller j.
     Refinement.  For every kept rung (pw_j, x_j, y_j) and every width pw in [pw_j - 7, pw_j + 7] that lies inside
       [wmin, wmax] and fits the frame with ph(pw): steps 2-7 of ssw_locate_rgb8 on the resize of S to pw x ph(pw), restricted
       to the candidate positions within +-8 of (x_j, y_j), clipped to the valid ones (a window that is empty after clipping
       contributes nothing).  A width shared by two kept rungs is resized once.
     Answer.  The (pw, ph, x, y, SAD) with the smallest SAD / (pw ph), compared by cross-multiplication in 64 bits
       (255 * 2^26 * 2^26 fits); ties: smaller pw, then y, then x.  host_sad[s] is its SAD.
   The rung step 8, the position stride 4, the box 8, the 8 kept rungs, +-7 and +-8 are fixed parts of the definition.
   Known limits: the aspect ratio is assumed kept and there is no rotation; smooth regions are ambiguous, and a smaller rung
   of a smooth patch can win on mean difference; min(pw, ph) >= 32 (enforced at wmin); an alpha channel is ignored.
   What runs: per (suspect, rung) one fused resize tile whose epilogue stores only T_j (R_j never reaches memory), the
   coarse kernel of ssw_locate_rgb8 on 2 x 2 phase planes of B8, and an atomic minimum of the key (D << 32) | position; every
   tap table of the ladder goes up in one copy.  The 8 kept rungs and the final comparison are chosen on the HOST: the call
   waits for the stream twice, after the ladder (8 bytes per rung come back) and for the answer, and the refinement's resizes
   use the context's cached tap tables like ssw_restore_rgb8 (one more wait per table that is new to the context).
   Workspace is grouped under the 256 MiB rule of ssw_locate_rgb8.  SSW_ERR_UNSUPPORTED: a rung's resize has no LDS tile
   of whole boxes (a rung about ten times smaller than the suspect).  Other status codes as ssw_locate_rgb8; n == 0: SSW_OK.
   Timed as SSW_STAGE_LOCATE, SSW_STAGE_LOCATE_COARSE (both coarse searches) and SSW_STAGE_RESIZE (rung tiles, refinement). */
typedef struct ssw_scale_range { uint32_t wmin, wmax; } ssw_scale_range;
int ssw_locate_scaled_rgb8(ssw_ctx* ctx, const uint8_t* dev_base_rgb, size_t w, size_t h, const void* const* dev_suspects,
                           ssw_placement* placements, const ssw_scale_range* ranges, size_t n, uint64_t* host_sad);
/* Diagnostic: T of ONE rung as the ladder's resize kernel stores it -- the (pw / 8) x (ph / 8) box means, row-major, of the
   luma of the suspect [sh][sw][channels] resized to pw x ph -- into host_boxes.  pw, ph >= 8.  Synchronises. */
int ssw_locate_rung_boxes(ssw_ctx* ctx, const void* dev_suspect, size_t sw, size_t sh, size_t channels, size_t pw, size_t ph,
                          uint8_t* host_boxes);

/* ---- locating a scaled cut-out whose aspect ratio was not kept exactly: a free height (csrc/locate_free.hip) ---- */
/* The scale ladder tries one height per width.  A thumbnail made for the web has both sides rounded on their own (480 x 333
   halves to 240 x 166, and ph(480) = 332), so the ladder's answer sits a row or a column off and the trace loses most of its
   similarity.  This call is the ladder followed by a full-resolution rescoring of the sizes near its answer, in both dimensions.
   pw, ph, x, y of each placement are OUTPUTS; w, h, channels are inputs; slack[s] = a, 1 <= a <= 4 (anything else:
   SSW_ERR_BAD_ARG).  Definition, per suspect S [sh][sw][c] against the original O [H][W][3]; everything is an integer, no sum
   depends on its order, and the result equals the numpy restatement in tests/test_locate_free_cpu.py exactly in pw, ph, x, y
   and SAD:
     1. A0 = (pw0, ph0, x0, y0) is exactly what ssw_locate_scaled_rgb8 answers for that suspect and range: every step and every
        constant of it stays as it is, and its status codes pass through.
     2. Sizes: every (pw, ph) with |pw - pw0| <= a, |ph - ph0| <= a, wmin <= pw <= wmax, min(pw, ph) >= 32, pw <= W, ph <= H.
        The height is free of the aspect rule.
     3. Positions, per size: x in [x0 - 4, x0 + 4] and [0, W - pw], y in [y0 - 4, y0 + 4] and [0, H - ph]; a window that is
        empty after clipping contributes nothing.
     4. SAD(pw, ph, x, y) = sum |L_R(i, j) - L_O(x + i, y + j)| over all pw ph pixels, with R and the luma of steps 1-2 of
        ssw_locate_rgb8: R = S when the size is the suspect's own, else the CatmullRom resize with the taps, clamping and
        rounding of csrc/resize_common.hpp.  An alpha channel is ignored.  No coarse pass and no top-8: every position of
        the window is scored in full.
     5. Answer: the smallest SAD / (pw ph), compared by cross-multiplication in 64 bits; ties: smaller pw, then smaller ph,
        then y, then x.  A0 is one of the candidates, so the answer's SAD per pixel is never above A0's.
   +-4 positions and the cap of 4 on a are fixed parts of the definition: at most 81 sizes x 81 positions per suspect.
   Known limits: aspect deviations beyond +-4 pixels are not searched; a deliberately squeezed picture is not this call's
   business; smooth regions stay ambiguous (as for ssw_locate_rgb8); there is no rotation.
   What runs: the ladder, then per (suspect, size) one fused resize tile (the front end of the ladder's rung kernel) whose
   epilogue sums the tile against the staged window of the original's luma plane: R is never stored.  Every tap table of the
   stage goes up in one copy; 32 (suspect, size) items per launch.  The final comparison runs on the HOST: the call waits for
   the stream three times, the ladder's two and once for the sums (81 x 8 bytes per size come back).  Workspace beyond the
   ladder's: the sums and the tap tables, a few hundred KiB.  SSW_ERR_UNSUPPORTED: a size whose resize has no LDS tile
   at all (the tile is chosen with the window counted, so no scale factor is refused for the window's sake).  Other status
   codes as ssw_locate_scaled_rgb8; n == 0: SSW_OK.  Timed as the ladder is, the stage itself as SSW_STAGE_LOCATE and
   SSW_STAGE_RESIZE (one kernel is both). */
int ssw_locate_free_rgb8(ssw_ctx* ctx, const uint8_t* dev_base_rgb, size_t w, size_t h, const void* const* dev_suspects,
                         ssw_placement* placements, const ssw_scale_range* ranges, const uint32_t* slack, size_t n,
                         uint64_t* host_sad);
/* Diagnostic: steps 2-5 of ssw_locate_free_rgb8 for ONE suspect [sh][sw][channels] from a start A0 = (pw0, ph0, x0, y0) the
   caller gives in place of the ladder's answer, every sum returned.  The same stage as the public call runs (the same items,
   launches and host comparison); a = slack.  host_sums [(2a + 1)^2][81], 64 bits each: SAD(pw, ph, x, y) lies at size slot
   (pw - pw0 + a) (2a + 1) + (ph - ph0 + a), position slot 9 (y - y0 + 4) + (x - x0 + 4) -- relative to the unclipped start, so
   the layout does not depend on the clipping.  Every slot that the definition does not score holds UINT64_MAX: a size dropped
   by wmin, wmax, 32, W or H, a position outside the clipped window, a window that is empty.  *answer (w, h, channels as given)
   and *host_sad are step 5; when no size is scored at all they are A0 and 0.  SSW_ERR_BAD_ARG: a null pointer, slack outside
   1 .. 4, channels not 3 or 4, a zero size, wmin > wmax (wmin below 32 is allowed: sizes stop at 32), a start the ladder never
   answers: pw0 == 0, ph0 == 0, pw0 > w, ph0 > h, x0 > w - pw0 or y0 > h - ph0.  SSW_ERR_UNSUPPORTED as for the public call.
   Waits for the stream once. */
int ssw_locate_free_sums_rgb8(ssw_ctx* ctx, const uint8_t* dev_base_rgb, size_t w, size_t h, const void* dev_suspect, size_t sw,
                              size_t sh, size_t channels, const uint32_t start[4] /* pw0, ph0, x0, y0 */, uint32_t wmin,
                              uint32_t wmax, uint32_t slack, uint64_t* host_sums, ssw_placement* answer, uint64_t* host_sad);

/* ---- identifying a suspect's original: an image catalogue searched on the device ---- */
/* Every stage above starts from "here is the original"; the finder of a leaked picture who owns a few thousand originals does
   not know which one it is.  These calls answer that, and so precede everything the reference's `test` command does with an
   original it is handed (the loop of examples/main.rs:369-415, Reader::base, src/algorithm.rs:462-464); the reference itself has
   no such step.  Everything is an integer, no sum depends on its order, and the results equal the numpy restatement in
   tests/test_identify_cpu.py exactly.
   Signature of a frame F [h][w][c] u8, c = 3 or 4, w, h >= 32:
     An alpha channel is ignored.  Luma is the one ssw_locate_rgb8 uses: L(p) = (77 R + 150 G + 29 B + 128) >> 8.
     The grid is 32 x 32.  Cell (i, j) covers x in [floor(i w / 32), floor((i + 1) w / 32)) and y in [floor(j h / 32),
     floor((j + 1) h / 32)); it is never empty, since w, h >= 32.
     sig[j][i] = (sum of L over the cell + n / 2) / n, n the cell's pixel count, integer division.  1024 bytes, row-major.
   Distance D(a, b) = sum_{t < 1024} |a[t] - b[t]|; at most 261 120, which fits 32 bits.
   Match of a query signature against a catalogue of nc signatures: the `top` entries (1 <= top <= 8) with the smallest
     (D, index) in lexicographic order -- ties go to the lower index; when nc < top the remaining slots hold index 0xFFFFFFFF and
     distance 0xFFFFFFFF.
   What it finds (measured with this definition on a 640 x 444 photograph, tests/test_identify_cpu.py): a marked copy of an
   original, as it is or resized anywhere between a tenth and one and a half times its size, re-encoded as JPEG or squeezed to
   another aspect ratio, lies at 2 900 .. 4 800 from its original, and every unrelated entry (the same picture rolled by 40
   columns included) at more than 15 000.
   Known limits: (1) a cut-out is NOT separable from unrelated images (a 580 x 404 cut-out of that photograph scores about
   13 000 against its own original, a zoomed crop about 15 000): cut-outs still need the original named, then ssw_locate_rgb8;
   (2) mirrored or turned copies do not match; (3) near-duplicates shifted by a pixel or two are not told apart.
   Timing: both calls are timed under SSW_STAGE_LOCATE (bytes); there is no stage of their own, because the number of stages
   is part of what callers and tests of this header rely on. */
typedef struct ssw_image_shape { uint32_t w, h, channels; } ssw_image_shape;
/* Signatures of n frames of DIFFERENT sizes and channel counts -> dev_sigs [n][1024].  dev_frames / shapes: HOST arrays of n
   device pointers / n shapes; frame i is [shapes[i].h][shapes[i].w][shapes[i].channels] u8.  No alignment is assumed of any
   pointer or of w * channels.  Only enqueues on the context's stream (no host wait; launch descriptors travel as kernel
   arguments, 32 frames per launch).  SSW_ERR_BAD_ARG: w or h < 32, channels not 3 or 4, a null pointer; SSW_ERR_UNSUPPORTED: a
   frame whose cells hold more than 2^24 pixels each; n == 0: SSW_OK. */
int ssw_signature_rgb8(ssw_ctx* ctx, const void* const* dev_frames, const ssw_image_shape* shapes, size_t n, uint8_t* dev_sigs);
/* The same on host images, one pointer per frame -> host_sigs [n][1024]: the frames are uploaded in groups of at most 256 MiB
   of workspace (one frame's own size if that is more), like the host forms of the trace, and the call returns when every
   buffer is the caller's again.  Bit-identical to the device form. */
int ssw_signature_host_rgb8(ssw_ctx* ctx, const uint8_t* const* host_frames, const ssw_image_shape* shapes, size_t n,
                            uint8_t* host_sigs);
/* Match nq query signatures dev_query [nq][1024] against nc catalogue signatures dev_catalogue [nc][1024]:
     dev_index [nq][top], dev_dist [nq][top]   the answer defined above, best first
     dev_all [nq][nc]                          (may be NULL) every distance
   Only enqueues on the context's stream.  The catalogue is read once per 128 queries and goes through the kernel in chunks
   of 32768 entries inside the call; indices are positions in dev_catalogue whatever the chunking.  No alignment is assumed.
   SSW_ERR_BAD_ARG: top outside 1 .. 8, nc >= 2^32, a null pointer; nq == 0: SSW_OK; nc == 0: SSW_OK with every slot at
   0xFFFFFFFF. */
int ssw_signature_match(ssw_ctx* ctx, const uint8_t* dev_query, size_t nq, const uint8_t* dev_catalogue, size_t nc, size_t top,
                        uint32_t* dev_index, uint32_t* dev_dist, uint32_t* dev_all);

/* ---- strength of a mark: its visibility and its collusion resistance (device-resident) ---- */
/* The two questions to answer before a copy ships: how far is a marked copy from its original, and how many recipients must
   pool their copies before tracing fails?  The second is the standard evaluation of a fingerprinting scheme and the reason
   the reference insists on N(0, 1) marks (src/algorithm.rs:604-606, Cox et al. IV-D) -- its own note on several marks in one
   image (src/algorithm.rs:389-393: 100 marks of N = 1000 leave each an average similarity of 3.1) is the nearest it comes
   to measuring it; the first is what the reference's README concedes for the default Option2(0.1) (a "cloudy" background).
   The reference computes neither.  Everything is an integer, no value depends on the order of a sum, and the results equal the
   numpy restatement in tests/test_collude_cpu.py exactly.  Both calls are timed under SSW_STAGE_CONVERT with their
   algorithmic bytes as work; there is no stage of their own, because the number of stages is part of what callers and tests
   of this header rely on.  Neither has a host-streaming form. */
/* Distance of n copies dev_copies [n][h][w][3] from their original(s) dev_base [n_base][h][w][3], n_base == 1 (the one
   original is compared against every copy) or n_base == n (frame i against copy i).  Per copy, with d = copy - base per byte
   and the luma of ssw_locate_rgb8, L(p) = (77 R + 150 G + 29 B + 128) >> 8:
     stats[0..2]  sum of d * d over the R, G and B bytes
     stats[3]     sum of (L(copy) - L(base))^2 over the pixels
     stats[4]     the number of bytes with d != 0
     stats[5]     max |d|
   dev_stats [n][6], 64 bits each (255^2 w h exceeds 32 bits from about 66 000 pixels).  PSNR is the caller's arithmetic:
   10 log10(255^2 * 3 w h / (stats[0] + stats[1] + stats[2])), infinite at 0.  The call zeroes dev_stats itself and only
   enqueues on the context's stream.  No alignment is assumed of any pointer or of w * 3.  With n_base == 1 a block reads its
   piece of the original once and goes over the copies with it: (1 + n) * 3 bytes per pixel.  Work: (n_base + n) * 3 w h +
   48 n bytes.  n == 0: SSW_OK; SSW_ERR_BAD_ARG: a null pointer, n_base not 1 or n; SSW_ERR_BAD_DIMS: w * h == 0 (and a side above
   2^31 or a frame whose bytes do not fit size_t, in both calls). */
int ssw_quality_rgb8(ssw_ctx* ctx, const uint8_t* dev_base, size_t n_base, const uint8_t* dev_copies, size_t n, size_t w, size_t h,
                     uint64_t* dev_stats);
/* A forged copy out of several: coalition i makes dev_out[i] [h][w][3] from `count` of the frames dev_copies [n_copies][h][w][3].
   The definition is per byte: v[j] are the values of the members at that byte in member order, s[0] <= ... <= s[c-1] the same
   values sorted, c = count; integer division throughout:
     SSW_COLLUDE_AVERAGE   (sum of v + c / 2) / c
     SSW_COLLUDE_MEDIAN    (s[(c-1)/2] + s[c/2] + 1) >> 1    -- odd c: the middle value itself
     SSW_COLLUDE_MIN       s[0]
     SSW_COLLUDE_MAX       s[c-1]
     SSW_COLLUDE_MINMAX    (s[0] + s[c-1] + 1) >> 1
     SSW_COLLUDE_MOSAIC    v[((x >> 5) + (y >> 5)) % c] at pixel (x, y): cut-and-paste of 32 x 32 tiles; the tile size is a
                           fixed part of the definition
   1 <= count <= 16; a member may occur more than once (a weighted coalition); count == 1 copies the frame.  `coalitions` is a
   HOST array; the descriptors travel as kernel arguments, 32 per launch as in ssw_restore_rgb8.  No host synchronisation, no
   workspace: the call only enqueues on the context's stream.  No alignment is assumed of any pointer or of w * 3.  dev_out
   must not overlap dev_copies.  Work: the sum over the coalitions of (c + 1) * 3 w h bytes.  n_coalitions == 0: SSW_OK;
   SSW_ERR_BAD_ARG: a null pointer, a count outside 1 .. 16, member >= n_copies, an unknown method (nothing is enqueued then);
   SSW_ERR_BAD_DIMS: an empty frame.
   What to expect (the oracle on a 640 x 444 photograph, k = 1000, alpha = 0.1, 8 copies; tests/test_collude_cpu.py): two
   colluders who average score 21.9 each and four 14.2, but three who take the median or the minimum already fall below 6. */
typedef enum ssw_collude_method {
    SSW_COLLUDE_AVERAGE = 0,
    SSW_COLLUDE_MEDIAN = 1,
    SSW_COLLUDE_MIN = 2,
    SSW_COLLUDE_MAX = 3,
    SSW_COLLUDE_MINMAX = 4,
    SSW_COLLUDE_MOSAIC = 5
} ssw_collude_method;
typedef struct ssw_coalition { uint32_t method, count; uint32_t member[16]; } ssw_coalition;
int ssw_collude_rgb8(ssw_ctx* ctx, const uint8_t* dev_copies, size_t n_copies, size_t w, size_t h, const ssw_coalition* coalitions,
                     size_t n_coalitions, uint8_t* dev_out);
/* The attack every leaked copy has been through -- somebody saved it as a JPEG: dev_out[j] [h][w][3] is frame jobs[j].frame of
   dev_frames [n_frames][h][w][3] as it comes back from a baseline JPEG of quality jobs[j].quality (1 .. 100), exactly what
   PIL's save(f, "JPEG", quality=q) followed by open gives (libjpeg-turbo's defaults).  Only the entropy coder, which loses nothing,
   is left out, so there is no bitstream and no file size.  The definition is in integers from end to end, and the numpy
   restatement in tests/test_jpeg_cpu.py (`jpeg_ref`, checked there against PIL byte for byte) is what the call equals:
     colour   Y = (19595 R + 38470 G + 7471 B + 32768) >> 16, Cb = (-11059 R - 21709 G + 32768 B + 8421375) >> 16,
              Cr = (32768 R - 27439 G - 5329 B + 8421375) >> 16  (8421375 = (128 << 16) + 32767)
     padding  to whole MCUs of 16 x 16 pixels: the luma, and the chroma's right edge, repeat the frame's last pixel; the chroma's
              bottom rows repeat the last DOWNSAMPLED row (of a frame of odd height: its last row is used twice first)
     4:2:0    Cb, Cr: the sum of 2 x 2 samples plus a bias that alternates 1, 2 along a row, >> 2
     tables   Annex K.1 (luma) and K.2 (chroma) times s percent, s = 5000 / q below quality 50 and 200 - 2 q from there on:
              (entry * s + 50) / 100 in integers, limited to 1 .. 255 (baseline); computed on the host
     blocks   per 8 x 8 block of samples - 128: jpeg_fdct_islow (rows, then columns; 13-bit constants), each coefficient divided
              by 8 * entry, round half away from zero, multiplied by entry again, jpeg_idct_islow (columns, then rows), + 128,
              limited to 0 .. 255
     upsample "fancy" h2v2: vertically 3 a + the sample above (even rows) or below (odd rows), then horizontally
              (3 c + left + 8) >> 4 for even and (3 c + right + 7) >> 4 for odd pixels, the frame's own first and last chroma
              sample repeated at the edges
     colour   R = Y + ((91881 Cr' + 32768) >> 16), G = Y + ((-22554 Cb' - 46802 Cr' + 32768) >> 16),
              B = Y + ((116130 Cb' + 32768) >> 16) with Cb' = Cb - 128, Cr' = Cr - 128, limited to 0 .. 255
   `jobs` is a HOST array; a frame may occur in many jobs and in any order.  The call only enqueues on the context's stream (no host
   synchronisation); the jobs go in groups of at most 16 whose decoded planes (1.5 bytes per padded pixel and job, at most 64 MiB
   or one job's) are the context's workspace, and their tables travel as kernel arguments.  No alignment is assumed of any
   pointer or of w * 3.  dev_out must not overlap dev_frames.  Timed under SSW_STAGE_CONVERT; work: per job 2 * 3 w h bytes of
   frames and 2 * (w h + 2 ceil(w / 2) ceil(h / 2)) bytes of planes.  n_jobs == 0: SSW_OK; SSW_ERR_BAD_ARG: a null pointer, a
   quality outside 1 .. 100, frame >= n_frames, a side below 8 (libjpeg's own upsampler reads beyond the last chroma column of
   frames 4 or fewer pixels wide; nothing is enqueued then); SSW_ERR_BAD_DIMS: an empty frame or a side above 65535, the most a
   JPEG holds.
   What to expect (the oracle on a 640 x 444 photograph, k = 1000; tests/test_jpeg_cpu.py): a copy marked at alpha 0.1 still
   scores 30.9 after quality 50 and 19.0 after quality 10; one marked at alpha 0.02 scores 20.6 after quality 50 and 3.7 --
   untraceable -- after quality 10.  Other subsampling modes, grey or CMYK frames, custom tables and the ifast / float DCTs are
   not offered. */
typedef struct ssw_jpeg_job { uint32_t frame; uint32_t quality; } ssw_jpeg_job;
int ssw_jpeg_rgb8(ssw_ctx* ctx, const uint8_t* dev_frames, size_t n_frames, size_t w, size_t h, const ssw_jpeg_job* jobs,
                  size_t n_jobs, uint8_t* dev_out);
/* A perceptual score beside PSNR: the structural similarity (SSIM) of n copies dev_copies [n][h][w][3] and their original(s)
   dev_base [n_base][h][w][3], n_base == 1 or n_base == n as in ssw_quality_rgb8.  Squared error is a poor measure of what a
   viewer sees -- eight copies of one photograph marked at one alpha spread over 8 dB of PSNR.  Luma is the one of
   ssw_locate_rgb8 / ssw_quality_rgb8, L(p) = (77 R + 150 G + 29 B + 128) >> 8; a is the luma of the original, b that of the copy.
     cells     4 x 4 pixels at (4 i, 4 j), i < floor(w / 4), j < floor(h / 4); the up to three trailing columns and rows take no part
     windows   8 x 8 pixels = 2 x 2 cells, at a stride of 4 pixels in both directions: nx = floor(w / 4) - 1 by
               ny = floor(h / 4) - 1 of them; window (wx, wy) covers the pixels [4 wx, 4 wx + 8) x [4 wy, 4 wy + 8)
   Per window, over its 64 pixels, all in 32-bit integers (the largest intermediate is 64 sum(a^2 + b^2) <= 532 684 800):
     s1 = sum a   s2 = sum b   ss = sum (a^2 + b^2)   s12 = sum a b
     vars  = 64 ss - s1^2 - s2^2          covar = 64 s12 - s1 s2
     n1 = 2 s1 s2 + 416                   n2 = 2 covar + 235963
     d1 = s1^2 + s2^2 + 416               d2 = vars + 235963
        (416 = floor(0.01^2 255^2 64 + .5), 235963 = floor(0.03^2 255^2 64 63 + .5))
     q = f64(n1 n2) / f64(d1 d2)          n1 n2 and d1 d2 exact in 64-bit integers (below 2^58), each converted
                                          round-to-nearest-even, one IEEE division
     t = (int32) floor(q 2^30 + 0.5)
   f64(n1) f64(n2) in place of the conversion of the exact product is the same number: the factors are exact in f64 and the
   product is rounded once.  In these integers 2 s1 s2 <= s1^2 + s2^2, vars - 2 covar = 64 sum (a - b)^2 - (s1 - s2)^2 >= 0 and
   d1 d2 > 0 hold exactly, so -2^30 < t <= 2^30 = SSW_SSIM_ONE, and t = 2^30 for every window of two equal frames.
   Per copy dev_stats [n][SSW_SSIM_STATS] receives two 64-bit values:
     stats[0]  the sum of t over all windows, signed
     stats[1]  the minimum over the windows of ((uint64)(t + 2^30) << 32 | index), index = wy nx + wx: the worst window; among
               equal windows the first one wins (one 64-bit atomic minimum: deterministic)
   and, when dev_map is not NULL, dev_map [n][ny][nx] receives t of every window.  The mean SSIM stats[0] / (2^30 nx ny) and the
   worst window's value and pixel position (4 wx, 4 wy) are the caller's arithmetic, as PSNR is for ssw_quality_rgb8.  Everything
   up to the division is an integer, the result is fixed-point and summed as integers: no value depends on the order of a sum,
   and the call equals the numpy restatement in tests/test_ssim_cpu.py (`ssim_ref`) exactly.
   The windows and constants are those of the widely used x264 / FFmpeg `ssim`; no bit equality with either is claimed (they
   evaluate in f32).  The limits: luma only; 8 x 8 box windows, not the Gaussian 11 x 11 of Wang et al.; trailing pixels ignored;
   no multi-scale variant; no host-streaming form.
   The call initialises dev_stats itself (sum 0, minimum all ones) and only enqueues on the context's stream, with no
   workspace.  No alignment is assumed of dev_base, dev_copies or of w * 3 (dev_stats and dev_map as their types require).  A
   block of the kernel owns SSW_SSIM_TILE_W x SSW_SSIM_TILE_H pixels of windows and reads one more column and row of cells;
   with n_base == 1 it reads them from the original once and goes over the copies: (1 + n) * 3 bytes per pixel, plus 8 % for the
   shared cells.  Timed under SSW_STAGE_CONVERT; work: (n_base + n) * 3 w h + 16 n bytes, + 4 nx ny n with a map.  n == 0: SSW_OK;
   SSW_ERR_BAD_ARG: a null dev_base, dev_copies or dev_stats, n_base not 1 or n, a side below SSW_SSIM_MIN_SIDE (nothing is
   enqueued then); SSW_ERR_BAD_DIMS: an empty frame, a side above 2^31, nx ny >= 2^32. */
enum { SSW_SSIM_MIN_SIDE = 8, SSW_SSIM_ONE = 1 << 30, SSW_SSIM_STATS = 2, SSW_SSIM_TILE_W = 252, SSW_SSIM_TILE_H = 60 };
int ssw_ssim_rgb8(ssw_ctx* ctx, const uint8_t* dev_base, size_t n_base, const uint8_t* dev_copies, size_t n, size_t w, size_t h,
                  uint64_t* dev_stats, int32_t* dev_map);
/* The attacks of a photo editor's filter menu: dev_out[j] [h][w][3] is frame jobs[j].frame of dev_frames [n_frames][h][w][3]
   after a Gaussian blur, an unsharp mask or a 3 x 3 median -- exactly what Pillow's ImageFilter.GaussianBlur(radius),
   UnsharpMask(radius, percent, threshold) and MedianFilter(3) give.  They are integer arithmetic on the bytes; the numpy
   restatement in tests/test_filter_cpu.py (`filter_ref`, checked there against Pillow byte for byte) is what the call equals.
   Every channel is filtered on its own.  clamp(i) = min(max(i, 0), n - 1) against the FRAME, applied anew in every pass.
     SSW_FILTER_BLUR(radius)   radius is the Gaussian's sigma, a float.  In float arithmetic, every operation rounded to float
              (the square root and the floor are taken in double and rounded), as Pillow's C does:
                s2 = radius * radius / 3          L = sqrt(12.0 * s2 + 1.0)          l = floor((L - 1.0) / 2.0)
                a = (2 l + 1) * (l * (l + 1) - 3 * s2)     a = a / (6 * (s2 - (l + 1) * (l + 1)))     rho = l + a
              then r = (int) rho, ww = (uint32) (16777216.0f / (rho * 2 + 1)), fw = (2^24 - (2 r + 1) ww) / 2 in integers.
              One box pass along a line of n samples:
                out[x] = (ww * sum_{|d| <= r} in[clamp(x + d)] + fw * (in[clamp(x - r - 1)] + in[clamp(x + r + 1)]) + 2^23) >> 24
              stored as a byte.  BLUR is three such passes along the rows, then three along the columns: six roundings to bytes.
              The weights sum to at most 2^24, so every intermediate fits 32 bits unsigned (at most 255 * 2^24 + 2^23).
              0 < radius <= 8.0 keeps r <= 7: a pass reaches 8 samples, three passes 24.  Radius 8.0: rho = 7.46875, r = 7,
              ww = 1052688, fw = 493448; radius 1.0: r = 0, ww = 11184811, fw = 2796202.  (r, ww, fw) are made on the host and
              travel as kernel arguments.
     SSW_FILTER_UNSHARP(radius, percent, threshold)   b = BLUR(radius) of the frame, d = in - b per byte; where |d| > threshold
              (strictly) out = min(max(in + d * percent / 100, 0), 255), the division truncating toward zero as in C; elsewhere
              out = in.  1 <= percent <= 1000, 0 <= threshold <= 255; Pillow's defaults are (2, 150, 3).
     SSW_FILTER_MEDIAN3   the fifth smallest of the 3 x 3 neighbourhood, indices clamped (the edge is repeated).
   Fields a kind does not use must be 0.  `jobs` is a HOST array; a frame may occur in many jobs and in any order; dev_out holds
   n_jobs frames in job order and must not overlap dev_frames.  The call only enqueues on the context's stream (no host
   synchronisation); the jobs go in groups of at most 16, and the row-blurred planes of a group's BLUR / UNSHARP jobs (3 bytes per
   pixel and job, at most 64 MiB or one job's) are the context's workspace.  No alignment is assumed of any pointer or of
   w * 3, and no minimum side: clamping defines everything from 1 x 1 on.  Timed under SSW_STAGE_CONVERT; work: per job
   2 * 3 w h bytes whatever the kind, one frame in and one out (a blur moves twice that, through the plane, and UNSHARP reads the
   frame once more).  n_jobs == 0 is checked first: SSW_OK; SSW_ERR_BAD_ARG: a null pointer, frame >= n_frames, an unknown kind,
   a radius outside (0, 8] or not finite, a percent outside 1 .. 1000, a threshold above 255, a non-zero unused field (nothing
   is enqueued when any job is bad); SSW_ERR_BAD_DIMS: a side of 0 or above 65535.
   Medians larger than 3 x 3, Pillow's kernel filters and BoxBlur, radii per axis, RGBA or grey frames are not offered. */
typedef enum ssw_filter_kind { SSW_FILTER_BLUR = 0, SSW_FILTER_UNSHARP = 1, SSW_FILTER_MEDIAN3 = 2 } ssw_filter_kind;
typedef struct ssw_filter_job { uint32_t frame; uint32_t kind; float radius; uint32_t percent; uint32_t threshold; } ssw_filter_job;
int ssw_filter_rgb8(ssw_ctx* ctx, const uint8_t* dev_frames, size_t n_frames, size_t w, size_t h, const ssw_filter_job* jobs,
                    size_t n_jobs, uint8_t* dev_out);
/* The scale attack: a copy scaled for the web.  ssw_resample_rgb8 makes of n_frames frames [h][w][3] the frames [nh][nw][3]
   that PIL.Image.resize((nw, nh), filter) makes of them -- exactly: Pillow's 8-bit resample is integer arithmetic on the bytes,
   and the numpy restatement in tests/test_resample_cpu.py (`resample_ref`, checked there against Pillow byte for byte) is what
   the call equals.  Every channel is resampled on its own.  One axis with `in` samples and `out` samples, in double on the
   host, each operation rounded on its own (no contraction; csrc/resample_tables.hpp):
       scale = in / out        fs = max(scale, 1.0)        support = S * fs        ss = 1 / fs
     and for output xx
       center = (xx + 0.5) * scale
       xmin = max((int) (center - support + 0.5), 0)              xmax = min((int) (center + support + 0.5), in) - xmin
       k[x] = f((x + xmin - center + 0.5) * ss)   for x < xmax    ww = sum of k in ascending order;  k[x] /= ww  if ww != 0
       tap[x] = (int) (k[x] * 2^22 - 0.5) if k[x] < 0, else (int) (k[x] * 2^22 + 0.5)          ((int) truncates toward zero)
     with the filters f and their supports S
       SSW_RESAMPLE_BOX       S = 0.5   1 for -0.5 < x <= 0.5, else 0
       SSW_RESAMPLE_BILINEAR  S = 1     1 - |x| for |x| < 1, else 0
       SSW_RESAMPLE_BICUBIC   S = 2     with a = -0.5 and x = |x|: ((a + 2) x - (a + 3)) x x + 1 for x < 1 (multiplied from the
                                        left); (((x - 5) x + 8) x - 4) a for 1 <= x < 2; else 0
       SSW_RESAMPLE_LANCZOS   S = 3     sinc(x) sinc(x / 3) for -3 <= x < 3, else 0; sinc(0) = 1, sinc(x) = sin(pi x) / (pi x)
                                        with libm's sin
     One pass along a line:   out[xx] = clip8((2^21 + sum_x in[xmin + x] * tap[x]) >> 22)
     with 32-bit sums (they are exact: the restatement asserts that each fits an int32), an arithmetic shift and a clamp to
     0 .. 255.  A frame is resampled along the rows first, into bytes, and then along the columns; a pass whose in == out is
     skipped, not run as an identity, and nw == w && nh == h is a copy.  Any w, h, nw, nh from 1 to 65535.  Pillow's NEAREST
     and HAMMING, `box`, `reducing_gap`, RGBA and 16-bit frames are not offered.
   ssw_scale_attack_rgb8 has the job signature of ssw_filter_rgb8: dev_out[j] [h][w][3] is frame jobs[j].frame of dev_frames
   [n_frames][h][w][3] resampled to jobs[j].nw x jobs[j].nh with jobs[j].filter as above, then brought back to w x h by the
   resize ssw_restore_rgb8 applies to a three-channel suspect of another size that covers the whole frame (the CatmullRom of
   csrc/resize_common.hpp, which ssw_resize_rgb8 shares): what a trace of the thumbnail sees.  nw == w && nh == h copies the
   frame.  `jobs` is a HOST array; a frame may occur in many jobs and in any order; consecutive jobs of one (nw, nh, filter) run
   as one batch.  The way back has the limits of ssw_restore_rgb8: SSW_ERR_UNSUPPORTED for a size that has no LDS tile (a
   thumbnail far larger than the frame), and the first use of a pair of lengths in a context waits for the stream once while
   its tap table goes up.
   Both calls only enqueue on the context's stream; their own tables go up in one copy per batch on that stream.  The row pass
   writes a byte plane [h][nw][3] per frame into the context's workspace, in groups of at most 32 frames and 64 MiB (or one
   frame's); the thumbnails of a batch live beside it, at most 64 MiB (or one job's) at a time.  No alignment is assumed of any
   pointer or of w * 3.  dev_out must not overlap the input.  Timed under SSW_STAGE_CONVERT; work per frame or job
   3 w h + 2 * 3 nw h + 3 nw nh bytes, the plane's term dropped when either pass is skipped; the way back of a job is timed as
   ssw_restore_rgb8 times it, under SSW_STAGE_RESIZE with 3 nw nh + 3 w h bytes.
   n_frames == 0 (resample) or n_jobs == 0 is checked first: SSW_OK; SSW_ERR_BAD_ARG: a null pointer, frame >= n_frames, an
   unknown filter, a dev_out that overlaps the input (nothing is enqueued when any job is bad); SSW_ERR_BAD_DIMS: a side of 0 or
   above 65535. */
typedef enum ssw_resample_filter {
    SSW_RESAMPLE_BOX = 0, SSW_RESAMPLE_BILINEAR = 1, SSW_RESAMPLE_BICUBIC = 2, SSW_RESAMPLE_LANCZOS = 3
} ssw_resample_filter;
int ssw_resample_rgb8(ssw_ctx* ctx, const uint8_t* dev_in, size_t n_frames, size_t w, size_t h, size_t nw, size_t nh, int filter,
                      uint8_t* dev_out);
typedef struct ssw_scale_job { uint32_t frame; uint32_t nw; uint32_t nh; uint32_t filter; } ssw_scale_job;
int ssw_scale_attack_rgb8(ssw_ctx* ctx, const uint8_t* dev_frames, size_t n_frames, size_t w, size_t h, const ssw_scale_job* jobs,
                          size_t n_jobs, uint8_t* dev_out);
/* The rotation attack and its undoing: a copy that was straightened or tilted in a photo editor, and what a tracer who knows
   the angle makes of it.  ssw_affine_rgb8 makes of n_frames frames in [h][w][3] the frames [oh][ow][3] that
   PIL.Image.transform((ow, oh), AFFINE, m, resample, fillcolor=fill) makes of them -- exactly: Pillow evaluates the transform
   in IEEE doubles, every operation rounded on its own (no contraction) and truncated to a byte, and the numpy restatement in
   tests/test_rotate_cpu.py (`affine_ref`, checked there against Pillow byte for byte) is what the call equals.
   The matrix, as PIL.Image.rotate(angle) makes it with expand=False and the default centre, in Python on the host
   (csrc/affine_tables.hpp: rotation_matrix makes the same numbers):
       a = -radians(angle % 360.0)
       m = [round(cos a, 15), round(sin a, 15), 0, round(-sin a, 15), round(cos a, 15), 0]
       cx, cy = w / 2.0, h / 2.0
       m[2] = (m[0] * -cx + m[1] * -cy + 0.0) + cx
       m[5] = (m[3] * -cx + m[4] * -cy + 0.0) + cy
   The transform: for output pixel (X, Y), every operation a double operation rounded on its own, in this order.
     1. Sample point.  xin = m0*(X+0.5) + m1*(Y+0.5) + m2 and yin = m3*(X+0.5) + m4*(Y+0.5) + m5, summed from the left.
     2. Outside test.  If xin < 0 || xin >= w || yin < 0 || yin >= h, the pixel is `fill`.  This test comes before any
        conversion to an integer.  (A sample point that is not a number -- the sums of a matrix with entries near the largest
        double can be one -- is outside as well; Pillow converts it.)
     3. Base position.  Otherwise xin -= 0.5; yin -= 0.5; x = floor(xin); y = floor(yin); dx = xin - x; dy = yin - y.
        XC(i) = clamp(i, 0, w-1) and YC(j) = clamp(j, 0, h-1).
     4. SSW_AFFINE_BILINEAR, per channel: L(a,b,d) = a + (b - a) * d.
          v1 = L(in[YC(y)][XC(x)], in[YC(y)][XC(x+1)], dx)
          v2 the same on row y+1 when 0 <= y+1 < h, otherwise v2 = v1
          v = L(v1, v2, dy); the byte is (uint8) v, truncated, with no +0.5.
     5. SSW_AFFINE_BICUBIC, per channel:
          C(a,b,c,d,t): p1 = b; p2 = -a + c; p3 = 2*(a - b) + c - d; p4 = -a + b - c + d; p1 + t*(p2 + t*(p3 + t*p4))
          r(j) = C(in[YC(j)][XC(x-1)], in[YC(j)][XC(x)], in[YC(j)][XC(x+1)], in[YC(j)][XC(x+2)], dx)
          v1 = r(y-1); v2 = r(y) if 0 <= y < h, otherwise v1; v3 = r(y+1) if 0 <= y+1 < h, otherwise v2;
          v4 = r(y+2) if 0 <= y+2 < h, otherwise v3; v = C(v1, v2, v3, v4, dy)
          the byte is 0 if v <= 0, 255 if v >= 255, otherwise (uint8) v, truncated.
   NEAREST, expand=True, another centre, `translate`, RGBA and 16-bit frames are not offered.  Pillow's own shortcuts for 0,
   180 and (on a square frame) 90 and 270 degrees are transposes; the formula gives them the same bytes (tests/test_rotate_cpu.py).
   The undoing is what a tracer who knows the angle would do.  F is the matrix of `angle` and B the matrix of `-angle`, both for
   the frame's own (w, h).  A is the attacked frame: the transform by F with the job's filter and fill.  U is the transform of
   A by B, always BICUBIC (the tracer does not know the attacker's filter).  O is the original.  The restored frame is U where
   the mask holds and O elsewhere -- the reference's recipe for lost pixels, "complement the attacked image with the original"
   (tests/attack_crop.rs).  The mask holds at (X, Y) when all three are true, (xin, yin) being B's sample point for (X, Y):
     - (xin, yin) is inside;
     - with x = floor(xin-0.5) and y = floor(yin-0.5) the footprint needs no clamping: x-1 >= 0, x+2 <= w-1, y-1 >= 0, y+2 <= h-1;
     - the sample points that F gives the four corner pixels of that footprint, (x-1 | x+2, y-1 | y+2), are all inside.
   Each term of the affine sum is monotone after rounding, so the corners bound every tap and no fill pixel of A is ever read
   under the mask: the restored frame does not depend on the fill.  A job whose forward and back are both the identity
   [1 0 0 0 1 0] (angle 0) is a copy of the frame, not a masked one.
   ssw_rotate_attack_rgb8: dev_out[j] [h][w][3] is frame jobs[j].frame of dev_frames [n_frames][h][w][3] attacked with
   jobs[j].forward, filter and fill, then undone with jobs[j].back over dev_base [h][w][3], the original.  ssw_unrotate_rgb8:
   dev_out[i] is suspect jobs[i].frame of dev_suspects [n][h][w][3] undone with jobs[i].back over dev_base, the mask made with
   jobs[i].forward; filter and fill are not read.  The undoing is one launch that writes no frame in between.  `jobs` is a HOST
   array; a frame may occur in many jobs and in any order; consecutive jobs of one filter, fill and pair of matrices run as one
   batch.  All three calls only enqueue on the context's stream.  The attacked frames of a batch live in the context's
   workspace, at most 32 jobs and 64 MiB (or one job's) at a time.  No alignment is assumed of any pointer or of w * 3.  Outputs
   must not overlap inputs.  Sides are 1 .. 65535.  The attack is timed under SSW_STAGE_CONVERT, the undoing under
   SSW_STAGE_RESIZE; work 3 w h + 3 ow oh bytes per transform.
   n_frames == 0, n_jobs == 0 or n == 0 is checked first: SSW_OK; SSW_ERR_BAD_ARG: a null pointer, an unknown filter,
   frame >= n_frames (unrotate: >= n), a matrix entry that is not finite, an output that overlaps an input (nothing is enqueued
   when any job is bad); SSW_ERR_BAD_DIMS: a side of 0 or above 65535.
   ssw_affine_plan is host arithmetic (no context): how a transform by m of a w x h frame would be launched -- *lds_form 1 when
   the box of source pixels of a tile of 32 x 8 output pixels (at most *box_w x *box_h; either may be null) is staged in LDS, 0
   when the taps come from global memory (a strong shrink or shear). */
typedef enum ssw_affine_filter { SSW_AFFINE_BILINEAR = 0, SSW_AFFINE_BICUBIC = 1 } ssw_affine_filter;
int ssw_affine_rgb8(ssw_ctx* ctx, const uint8_t* dev_in, size_t n_frames, size_t w, size_t h, size_t ow, size_t oh, const double* m,
                    int filter, const uint8_t* fill, uint8_t* dev_out);
typedef struct ssw_rotate_job { uint32_t frame, filter; uint8_t fill[4]; double forward[6], back[6]; } ssw_rotate_job;
int ssw_rotate_attack_rgb8(ssw_ctx* ctx, const uint8_t* dev_base, const uint8_t* dev_frames, size_t n_frames, size_t w, size_t h,
                           const ssw_rotate_job* jobs, size_t n_jobs, uint8_t* dev_out);
int ssw_unrotate_rgb8(ssw_ctx* ctx, const uint8_t* dev_base, const uint8_t* dev_suspects, size_t n, size_t w, size_t h,
                      const ssw_rotate_job* jobs, uint8_t* dev_out);
/* How much of a w x h frame an undoing takes from the rotated copy: host_kept[i] (a HOST array of n) is the number of pixels
   under the mask of jobs[i] (forward and back are read; an identity job: all w h).  Counted on the device, one launch per job;
   waits for the context's stream.  n == 0: SSW_OK; SSW_ERR_BAD_ARG: a null pointer, a matrix entry that is not finite;
   SSW_ERR_BAD_DIMS: a side of 0 or above 65535. */
int ssw_unrotate_kept(ssw_ctx* ctx, size_t w, size_t h, const ssw_rotate_job* jobs, size_t n, uint64_t* host_kept);
int ssw_affine_plan(size_t w, size_t h, const double* m, int* lds_form, uint32_t* box_w, uint32_t* box_h);
/* PIL.Image.rotate(angle)'s matrix for a w x h frame as stated above, number for number what Python makes (host arithmetic, no
   context; tests/test_rotate_cpu.py compares 64 angles bit for bit).  SSW_ERR_BAD_ARG: m null or an angle that is not finite. */
int ssw_rotation_matrix(double angle, size_t w, size_t h, double* m);

/* ---- finding the angle of a turned copy: an angle ladder (csrc/angle.hip) ------------------------------------------------
   By which angle was each suspect turned?  A search over the angle of a rotation about the centre -- what PIL.Image.rotate
   does without `expand` -- for suspects of the original's size.  Everything is an integer and no sum depends on its order:
   the answer equals the numpy restatement of tests/test_angle_cpu.py exactly.  The reference has no counterpart.
   Inputs.  The original O = dev_base and n suspects S = dev_suspects [n], all [h][w][3] u8.  A range amin <= amax in degrees,
   counter-clockwise as PIL.Image.rotate, -45 <= amin, amax <= 45.
   Angles.  Every angle is a / 32 degrees for an integer a (an exact double).  Of the matrix that ssw_rotation_matrix makes for
   a / 32 the search uses C(a) = floor(m0 * 65536 + 0.5) and S(a) = floor(m1 * 65536 + 0.5), evaluated in doubles, and nothing
   else: ssw_angle_table gives the two (host arithmetic, no context; SSW_ERR_BAD_ARG: a null pointer).
   Planes.  L = (77 R + 150 G + 29 B + 128) >> 8, the luma of ssw_locate_rgb8.  f = 1: the planes Po (original) and Ps (suspect)
   are L itself, wr = w, hr = h.  f = 4: the decimated 4 x 4 box means (sum + 8) >> 4 at (4 X, 4 Y), wr = w >> 2, hr = h >> 2
   (trailing pixels are dropped).
   Cost of angle a at factor f (64-bit integers; lg = log2 f, sh = 17 + lg).  For every pixel (X, Y) of Ps:
       p  = 2 f X + f - w                          q  = 2 f Y + f - h          (half pixels of the frame from its centre)
       Rx = (w - f) * 65536 + C p + S q            Ry = (h - f) * 65536 - S p + C q
       X0 = Rx >> sh, fx = (Rx >> (sh - 8)) & 255; Y0, fy likewise of Ry                      (arithmetic shifts)
       valid = 1 <= X0 <= wr - 3 and 1 <= Y0 <= hr - 3
       v  = ((256-fx)(256-fy) Po[Y0][X0] + fx (256-fy) Po[Y0][X0+1] + (256-fx) fy Po[Y0+1][X0] + fx fy Po[Y0+1][X0+1] + 32768) >> 16
   D = sum over the valid pixels of |Ps[Y][X] - v|, c = their number: the original's plane turned forward by the candidate
   against the suspect as it is.  Mean costs are compared cross-multiplied in 64 bits: (D1, c1) < (D2, c2) when D1 c2 < D2 c1.
   Ladder.  j0 = floor(4 amin), j1 = ceil(4 amax), clipped to -180 .. 180; one rung per j in j0 .. j1: the angle a = 8 j (a step
   of 0.25 degrees) at f = 4.  Kept: the 4 rungs of smallest mean cost, ties to the smaller j (all, when there are fewer).
   Refinement: every a within 7 of a kept rung's 8 j and inside 8 j0 .. 8 j1, each once, at f = 1.  Answer: the smallest mean
   cost of the refinement, ties to the smaller a.
   host_found[i] (a HOST array of n): n = the answer a of suspect i (its angle is n / 32 degrees), sad and count = its D and c,
   n_rungs = j1 - j0 + 1.  host_rungs (a HOST array, may be null): [n][n_rungs][2] = D, c of every rung of every suspect.
   The original's planes are made once per call; the suspects go in groups of at most 256 MiB of planes (one suspect's, if
   they are larger).  The kept rungs are chosen on the device: the call waits for the context's stream once, at its end (the
   answer is needed on the host).  Timed under SSW_STAGE_LOCATE; the ladder's launch -- the coarse pass -- also under
   SSW_STAGE_LOCATE_COARSE (work: byte differences), as ssw_locate_rgb8 bills its own.
   n == 0 is checked first: SSW_OK.  SSW_ERR_BAD_ARG: a null pointer, a range that is not finite, reversed or beyond +-45;
   SSW_ERR_BAD_DIMS: a side below 32 (with this limit c > 0 at every angle of the range); SSW_ERR_UNSUPPORTED: w h > 2^27
   (the cross-multiplied products stay below 2^63).  Not searched: a copy that was turned AND scaled; a copy that was turned and
   cropped, or turned about another centre, is ssw_locate_turned_rgb8's.  The answer's resolution is 1/32 degree. */
typedef struct ssw_angle_found { int32_t n; uint32_t n_rungs; uint64_t sad, count; } ssw_angle_found;
int ssw_find_angle_rgb8(ssw_ctx* ctx, const uint8_t* dev_base, const uint8_t* dev_suspects, size_t n, size_t w, size_t h,
                        double amin, double amax, ssw_angle_found* host_found, uint64_t* host_rungs);
int ssw_angle_table(int32_t n, int32_t* c, int32_t* s);

/* ---- the rotation attack undone by the angle FOUND: the strength report's unknown-angle row (csrc/angle.hip) -----------------
   What does a turn leave of the mark when the tracer is NOT told the angle?  Job i is defined entirely by calls above:
     T_i       = what ssw_affine_rgb8 makes of frame jobs[i].frame of dev_frames [n_frames][h][w][3] with jobs[i].forward, filter
                 and fill at the frame's own size -- the first half of ssw_rotate_attack_rgb8.  jobs[i].back is NOT read.
     found_i   = what ssw_find_angle_rgb8(dev_base, T_i, amin, amax) answers: host_found[i] (n, n_rungs, sad, count) and, when
                 host_rungs (a HOST array, may be null) is given, [n_jobs][n_rungs][2] = D, c of every rung.  Ladder, the 4 kept
                 rungs, tie rules and refinement are that call's; no constant differs.
     dev_out[i] [h][w][3] = what ssw_unrotate_rgb8 makes of T_i over dev_base for the job whose forward is
                 ssw_rotation_matrix(n_i / 32, w, h) and whose back is ssw_rotation_matrix(-n_i / 32, w, h): turned back by the
                 angle found and completed with the original (n_i = 0: a copy of T_i).
     host_kept[i] (a HOST array of n_jobs) = what ssw_unrotate_kept counts for that job.
     dev_turned (may be null): [n_jobs][h][w][3] receives T_i.
   What runs.  All suspects of the call have one original, and the cost of an angle turns the ORIGINAL forward: the turned values
   depend on (original, angle) only.  Jobs whose forward matrices are equal form share-groups of at most 16; angle_cost_shared_kernel
   makes the turned values of a (tile, candidate angle) once and compares them with every member that wants the candidate -- in the
   ladder every member wants every rung, in the refinement the candidates of a group are the union of its members' lists and a
   member's sums go to its own slots only, so a neighbour never changes an answer.  The sums are integers: host_found and the
   rungs EQUAL ssw_find_angle_rgb8's.  Jobs go in groups whose turned frames and planes are at most 256 MiB (one job's, if they
   are larger); the call waits for the context's stream TWICE per group -- for the slot lists, of which the host forms the unions,
   and for the answers, which shape the undoing -- and once more at its end (rung sums, kept counts), whatever the number of
   suspects or angles.  Timed under SSW_STAGE_LOCATE / SSW_STAGE_LOCATE_COARSE (planes, ladder, refinement) and SSW_STAGE_RESIZE
   (the turn and its undoing).
   n_jobs == 0 is checked first: SSW_OK.  SSW_ERR_BAD_ARG: a null pointer (dev_turned and host_rungs excepted), a range that is
   not finite, reversed or beyond +-45, frame >= n_frames, a filter that is not an ssw_affine_filter, a forward entry that is not
   finite, an output that overlaps an input or the other output; SSW_ERR_BAD_DIMS: a side below 32 or above 65535;
   SSW_ERR_UNSUPPORTED: w h > 2^27. */
int ssw_rotate_search_attack_rgb8(ssw_ctx* ctx, const uint8_t* dev_base, const uint8_t* dev_frames, size_t n_frames, size_t w, size_t h,
                                  const ssw_rotate_job* jobs, size_t n_jobs, double amin, double amax, uint8_t* dev_out,
                                  uint8_t* dev_turned, ssw_angle_found* host_found, uint64_t* host_rungs, uint64_t* host_kept);

/* ---- locating cut-outs of a turned copy: angle and position together (csrc/locate_turned.hip) --------------------------------
   "Straighten by a degree" turns a picture and crops the wedges away: what reaches the tracer is a cut-out of a turned frame,
   its angle and its position both unknown.  Everything is an integer and no sum depends on its order: the answer equals the
   numpy restatement of tests/test_locate_turned_cpu.py exactly.  The reference has no counterpart.
   Inputs.  The original O = dev_base [h][w][3] u8, here W x H; per suspect S = dev_suspects[i] [sh][sw][3] u8, shapes[i] =
   (sw, sh, channels).  A range amin <= amax in degrees, counter-clockwise as PIL.Image.rotate, within +-45.  The suspect is
   taken to be an axis-aligned crop of the original's frame turned about any centre, at the original's scale and without any of
   the attacker's fill.
   Angles and planes.  An angle is n / 32 degrees; C(n), S(n) are those of ssw_angle_table.  Lo, Ls: the luma
   (77 R + 150 G + 29 B + 128) >> 8 of O and S.
   Template of angle n at size tw x th: the suspect's luma turned back about its own centre.  For 0 <= X < tw, 0 <= Y < th
   (64-bit integers, arithmetic shifts):
       p  = 2 X + 1 - tw                           q  = 2 Y + 1 - th
       Rx = (sw - 1) * 65536 + C p - S q           Ry = (sh - 1) * 65536 + S p + C q
       X0 = Rx >> 17, fx = (Rx >> 9) & 255; Y0, fy likewise of Ry
       T(X, Y) = ((256-fx)(256-fy) Ls[Y0][X0] + fx (256-fy) Ls[Y0][X0+1] + (256-fx) fy Ls[Y0+1][X0] + fx fy Ls[Y0+1][X0+1] + 32768) >> 16
   A pixel is valid when 0 <= X0 <= sw - 2 and 0 <= Y0 <= sh - 2.
   Template size of angle n: the largest i in 1 .. sw / 8 for which the four corner pixels of the template tw = 8 i,
   th = 8 max(1, (2 i sh + sw) / (2 sw)) are valid.  Rx and Ry are monotone in X and in Y, so the corners bound every tap: every
   pixel of a template is valid.  The angle is dropped when there is no such i, when min(tw, th) < 32, when tw > W or th > H.
   Ladder.  j0 = floor(4 amin), j1 = ceil(4 amax); one rung per j, at the angle n = 8 j.  T_j: the 8 x 8 box means (sum + 32) >> 6
   of the rung's template at multiples of 8.  B8: the box means of Lo of ssw_locate_scaled_rgb8, at every multiple of 4.
   D_j(x, y) = sum |T_j(i, k) - B8(x + 8 i, y + 8 k)| at the candidate positions x <= W - tw, y <= H - th that are multiples of 4.
   The rung's entry is its smallest (D, y, x); n_j = (tw / 8)(th / 8).
   Kept: the 4 rungs of smallest D_j / n_j (all, when fewer are left), compared cross-multiplied in 64 bits, ties to the smaller j;
   dropped rungs are never kept.
   Refinement.  Every n within 7 of a kept rung's 8 j and inside 8 j0 .. 8 j1, each once: an angle within 7 of two kept rungs
   belongs to the one of better rank.  A dropped angle is passed over.  For n, its own template tw_n x th_n at full resolution
   takes steps 2-7 of ssw_locate_rgb8 (as the luma of R), the positions restricted to those within +-8 of
   ((2 x_j + tw_j - tw_n) >> 1, (2 y_j + th_j - th_n) >> 1), clipped to the frame; an angle whose window is empty after the
   clipping is passed over (the rung's own angle never is).
   Answer.  The smallest SAD / (tw th), compared cross-multiplied; ties to the smaller n, then y, then x.  host_found[i] (a HOST
   array of n): n, x, y, tw, th, sad and n_rungs = j1 - j0 + 1.  The suspect's centre lies at (2 x + tw, 2 y + th) half pixels of
   the original, its angle is n / 32 degrees.  host_rungs (a HOST array, may be null): [n][n_rungs][4] = D, n_j, x, y of every
   rung's entry, a dropped rung all zero.
   The suspects go in groups of at most 256 MiB of luma planes (one suspect's, if larger); a launch holds at most 32 rungs and
   256 MiB of boxes and differences; the refinement's templates go 256 MiB at a time.  The kept rungs are chosen on the host:
   a group waits for the context's stream twice -- for the ladder's minima and for the answer -- and once more for every
   further 256 MiB of templates.  Templates are timed under SSW_STAGE_RESIZE, the searches under SSW_STAGE_LOCATE and
   SSW_STAGE_LOCATE_COARSE as ssw_locate_scaled_rgb8 bills its own.
   n == 0 is checked first: SSW_OK.  SSW_ERR_BAD_ARG: a null pointer, channels other than 3 or 4, a range that is not finite,
   reversed or beyond +-45; SSW_ERR_BAD_DIMS: a side of 0 or above 65535, every rung of a suspect dropped;
   SSW_ERR_UNSUPPORTED: 4 channels, 2^32 or more candidate positions.  Not searched: a cut-out that was scaled as well, one
   that holds the attacker's fill.  The answer's position grid is one pixel (the centre half a pixel): a half-pixel refinement
   of the centre is the step after.
   ssw_locate_turned_rung_boxes: *tw, *th = the template size of angle n (-1440 .. 1440) for a suspect sw x sh, and, unless
   host_boxes is null, host_boxes [th / 8][tw / 8] = its T_j as the device makes it (for tests; waits for the stream).
   SSW_ERR_BAD_ARG: a null pointer, n out of range; SSW_ERR_BAD_DIMS: a side of 0 or above 65535, no valid size. */
typedef struct ssw_turned_shape { uint32_t w, h, channels; } ssw_turned_shape;
typedef struct ssw_turned_found { int32_t n; uint32_t x, y, tw, th, n_rungs; uint64_t sad; } ssw_turned_found;
int ssw_locate_turned_rgb8(ssw_ctx* ctx, const uint8_t* dev_base, size_t w, size_t h, const void* const* dev_suspects,
                           const ssw_turned_shape* shapes, size_t n, double amin, double amax, ssw_turned_found* host_found,
                           uint64_t* host_rungs);
int ssw_locate_turned_rung_boxes(ssw_ctx* ctx, const void* dev_suspect, size_t sw, size_t sh, int32_t n, uint32_t* tw, uint32_t* th,
                                 uint8_t* host_boxes);
/* Restoring a cut-out of a turned copy whose angle and centre are known (found by ssw_locate_turned_rgb8, or given): what a
   tracer does with it before ssw_fingerprint_trace.  jobs[i] = (angle, cx, cy) in doubles for suspect i: turned by `angle`
   degrees, its centre at (cx, cy) pixels of the original; the found ones are n / 32, x + tw / 2.0 and y + th / 2.0.  b is the
   matrix of ssw_rotation_matrix(-angle, ...), of which only the entries 0, 1, 3 and 4 are used, and
       m = [b0, b1, (b0 * -cx + b1 * -cy + 0.0) + sw / 2.0, b3, b4, (b3 * -cx + b4 * -cy + 0.0) + sh / 2.0],
   every operation rounded on its own.  dev_out[i] [h][w][3]: a pixel is what PIL.Image.transform((w, h), AFFINE, m, BICUBIC)
   makes of the suspect -- the arithmetic of ssw_affine_rgb8, steps 1-3 and 5 -- where the sample point is inside the suspect and
   the footprint needs no clamping (x-1 >= 0, x+2 <= sw-1, y-1 >= 0, y+2 <= sh-1); elsewhere the original's pixel stands, the
   reference's recipe for lost pixels as in ssw_unrotate_rgb8.  The restored frames equal `restore_turned_ref` of
   tests/test_locate_turned_cpu.py byte for byte.  One launch per suspect, no frame in between; only enqueues on the context's
   stream; timed under SSW_STAGE_RESIZE (work 3 sw sh + 3 w h bytes per suspect).
   n == 0 is checked first: SSW_OK.  SSW_ERR_BAD_ARG: a null pointer, channels other than 3 or 4, a job that is not finite, an
   output that overlaps an input; SSW_ERR_BAD_DIMS: a side of 0 or above 65535; SSW_ERR_UNSUPPORTED: 4 channels. */
typedef struct ssw_turned_job { double angle, cx, cy; } ssw_turned_job;
int ssw_restore_turned_rgb8(ssw_ctx* ctx, const uint8_t* dev_base, size_t w, size_t h, const void* const* dev_suspects,
                            const ssw_turned_shape* shapes, const ssw_turned_job* jobs, size_t n, uint8_t* dev_out);

/* ---- the crop attack: a part of the picture, placed or searched, also scaled (csrc/crop.hip) ----------------------------------
   The reference's second robustness test cuts a rectangle out of the marked copy and lays it over the original again
   (tests/attack_crop.rs:56-70); the most common leaked copy is such a part that was also scaled for the web.  Both calls make the
   frames a trace of such a copy sees, and both are defined entirely by calls above.  Job j, with F = frame jobs[j].frame of
   dev_frames [n_frames][h][w][3]:
     C_j   = the rectangle (x, y, cw, ch) of F as a dense frame [ch][cw][3].
     T_j   = C_j when tw = th = 0, else what ssw_resample_rgb8(C_j, cw, ch, tw, th, filter) makes of it: Pillow's
             crop((x, y, x + cw, y + ch)).resize((tw, th), filter), byte for byte.
     ssw_crop_attack_rgb8 (placed: the tracer is told the rectangle)
       dev_out[j] [h][w][3] = what ssw_restore_rgb8(dev_base, T_j, {w, h of T_j, 3, x, y, cw, ch}) makes: T_j brought back to
             cw x ch by the CatmullRom of csrc/resize_common.hpp when it was scaled, and the original everywhere else.
     ssw_crop_search_attack_rgb8 (searched: the tracer's own search says where the piece came from)
       host_found[j], host_sad[j] = for searches[j] = (0, 0) what ssw_locate_rgb8(dev_base, T_j) answers for the piece at its own
             size (pw, ph are filled in with T_j's w, h); otherwise what ssw_locate_scaled_rgb8(dev_base, T_j, {wmin, wmax})
             answers.  Definition, tie rules and every constant are those calls'; none differs.
       dev_out[j] = what ssw_restore_rgb8(dev_base, T_j, host_found[j]) makes.
     dev_thumbs (may be null) receives the T_j packed one behind the other, in job order, 3 tw th (or 3 cw ch) bytes each.
   What runs.  The resizes, the searches and the restore of a scaled or searched piece ARE the calls named, made inside the
   library on the pieces where they lie; consecutive jobs of one (cw, ch, tw, th, filter) are one ssw_resample_rgb8 call, the
   searches of a group one ssw_locate_rgb8 and one ssw_locate_scaled_rgb8 call.  Two kernels are new.  crop_cut_kernel makes the
   C_j that a resize or a search reads (and the T_j of an unscaled job when dev_thumbs asks for it).  crop_complement_kernel makes
   dev_out[j] of a placed, unscaled job in one pass -- every output row is the original's bytes, the copy's, the original's -- so
   no piece is written and read back: it equals cut + ssw_restore_rgb8 byte for byte.  Neither assumes an alignment of any
   pointer, of 3 x or of 3 w.
   Jobs run in groups, in the order of the call, whose pieces and thumbnails in the context's workspace are at most 256 MiB (one
   job's, if they are more); with dev_thumbs the thumbnails lie there and only the pieces of scaled jobs count.
   ssw_crop_attack_rgb8 only enqueues on the context's stream, apart from the wait ssw_restore_rgb8 has for a tap table
   (cw <- tw, ch <- th) the context has not cached; those tables go up before anything is enqueued.
   ssw_crop_search_attack_rgb8 waits as the locate calls do, PER GROUP: once for the group's (0, 0) searches if it has any
   (ssw_locate_rgb8), twice for its ranged searches if it has any (ssw_locate_scaled_rgb8: after the ladder and for the answer),
   and once more per tap table that is new to the context (the refinement's and the restore's).
   Timed under the stages of the parts: the cuts as SSW_STAGE_CONVERT (6 bytes per pixel of a piece), the resamples as
   SSW_STAGE_CONVERT, the complement and the restores as SSW_STAGE_RESIZE (the complement: 6 w h bytes per job), the searches as
   SSW_STAGE_LOCATE / SSW_STAGE_LOCATE_COARSE.  A call of placed, unscaled jobs without dev_thumbs bills SSW_STAGE_RESIZE alone.
   n_jobs == 0 is checked first: SSW_OK.  SSW_ERR_BAD_ARG: a null pointer (dev_thumbs excepted), frame >= n_frames, cw or ch of 0,
   a rectangle that leaves the frame, one of tw, th zero and the other not, an unknown filter of a scaled job, an output that
   overlaps an input or the other output; SSW_ERR_BAD_DIMS: w or h of 0, a side above 65535.  Nothing is enqueued then.  The
   status codes of the parts come through as they are (ssw_locate_scaled_rgb8: SSW_ERR_BAD_ARG for a range that leaves no rung
   or has min(wmin, ph(wmin)) < 32; SSW_ERR_UNSUPPORTED for a resize that has no LDS tile); the groups before the failing one
   have run. */
typedef struct ssw_crop_job { uint32_t frame, x, y, cw, ch, tw, th, filter; } ssw_crop_job;      /* tw = th = 0: not scaled */
int ssw_crop_attack_rgb8(ssw_ctx* ctx, const uint8_t* dev_base, const uint8_t* dev_frames, size_t n_frames, size_t w, size_t h,
                         const ssw_crop_job* jobs, size_t n_jobs, uint8_t* dev_out, uint8_t* dev_thumbs);
typedef struct ssw_crop_search { uint32_t wmin, wmax; } ssw_crop_search;                         /* 0, 0: the piece's own size */
int ssw_crop_search_attack_rgb8(ssw_ctx* ctx, const uint8_t* dev_base, const uint8_t* dev_frames, size_t n_frames, size_t w, size_t h,
                                const ssw_crop_job* jobs, const ssw_crop_search* searches, size_t n_jobs, uint8_t* dev_out,
                                uint8_t* dev_thumbs, ssw_placement* host_found, uint64_t* host_sad);

/* ---- 16-bit frames (device-resident, batched) ----------------------------------- */
/* `DynamicImage::into_rgb32f()` for 16-bit input (ImageRgb16; call sites src/algorithm.rs:308, :476): v / 65535,
   and `into_rgb16()` from Rgb32F: round(clamp(v,0,1) * 65535) (`image 0.24.3`, like the 8-bit forms). */
int ssw_convert_rgb16_to_f32(ssw_ctx* ctx, const uint16_t* dev_in, size_t n_values, float* dev_out);
int ssw_convert_f32_to_rgb16(ssw_ctx* ctx, const float* dev_in, size_t n_values, uint16_t* dev_out);
/* ssw_batch_embed / ssw_batch_extract on 16-bit frames: v / 65535 fused into the first operand pre-pass (6 instead of
   12 B/px read at the boundary).  The marked frames come back as f32 -- what Writer::mark returns
   (src/algorithm.rs:355-379: Rgb32F); quantise with ssw_convert_f32_to_rgb16 / _rgb8 as the caller would.  Bit-identical
   to the f32 entry points on host-converted frames.  Same reference lines as the f32 forms. */
int ssw_batch_embed_rgb16(ssw_ctx* ctx, const ssw_config* cfg, const uint16_t* dev_rgb, size_t n_frames,
                          size_t w, size_t h, const float* dev_marks, size_t k, float* dev_rgb_out);
int ssw_batch_extract_rgb16(ssw_ctx* ctx, const ssw_config* cfg, const uint16_t* dev_base_rgb,
                            const uint16_t* dev_derived_rgb, size_t n_frames, size_t w, size_t h, size_t k,
                            float* dev_extracted, const float* dev_marks, float* dev_sims);

/* ---- host-image streaming (n frames that live on the host, one call) ------------- */
/* The loops of the reference's callers -- examples/main.rs:271-278 (`watermark`: per image Writer::new -> mark ->
   into_rgb8) and :383-415 (`test`: per image Reader::base / derived -> extract -> Tester::similarity) -- as ONE call over
   n 8-bit host images [h][w][3] (frames[i]: one pointer per image; pinned buffers -- ssw_host_alloc, hipHostRegister --
   are the DMA source / target themselves, any other buffer goes through the context's staging ring): the images go
   through ssw_batch_embed_rgb8 / ssw_batch_extract_rgb8 in groups of frames (G = 8 4K frames by default; a call ramps
   up through groups of G/4 and G/2 frames, embed ramps down again), the upload of group g + 1, the kernels of group g
   and the download of group g - 1 in flight together (csrc/ssw_stream.hip).  The output side overlaps fully only
   with pinned output buffers (a pageable buffer is filled by a blocking staged copy; it is issued after the next
   group's kernels are queued, so the device keeps working, but the host thread sleeps in it).  The device ring of a
   call (3 slots x 2 buffers of G frames) stays allocated until ssw_ctx_destroy or until an allocation of the context
   runs short of device memory.  Bit-identical to the single-image handles.  Host-buffer entry points: they return when every buffer is the caller's again.
   host_marks: [n][k] f32 (mark i for frame i); extract: host_marks and host_sims both or neither (NULL). */
int ssw_batch_embed_host_rgb8(ssw_ctx* ctx, const ssw_config* cfg, const uint8_t* const* host_frames, size_t n_frames,
                              size_t w, size_t h, const float* host_marks, size_t k, uint8_t* const* host_out);
int ssw_batch_extract_host_rgb8(ssw_ctx* ctx, const ssw_config* cfg, const uint8_t* const* host_base,
                                const uint8_t* const* host_derived, size_t n_frames, size_t w, size_t h, size_t k,
                                float* host_extracted, const float* host_marks, float* host_sims);

/* ---- single-image handles mirroring the crate's types (host buffers) ------- */
/* Writer::new(image, config), src/algorithm.rs:295-316.  rgb_hwc: host [h][w][3]
   f32 (what `into_rgb32f()` yields, :308).  The ordering is computed lazily at
   embed time, when the mark length is known (only the first k entries are ever
   consumed, :396). */
int ssw_writer_create(ssw_ctx* ctx, const float* rgb_hwc, size_t w, size_t h,
                      const ssw_config* cfg, ssw_writer** out);
/* Writer::new on an 8-bit image: `image.into_rgb32f()` (src/algorithm.rs:308; v / 255) happens on the
   device, fused into the colour conversion, and 3 instead of 12 bytes per pixel cross PCIe.  rgb_hwc:
   host [h][w][3] u8.  Bit-identical to ssw_writer_create on the host-converted frame. */
int ssw_writer_create_rgb8(ssw_ctx* ctx, const uint8_t* rgb_hwc, size_t w, size_t h,
                           const ssw_config* cfg, ssw_writer** out);
/* Writer::new on a 16-bit image (ImageRgb16): `into_rgb32f()` (src/algorithm.rs:308; v / 65535) on the device, 6 instead
   of 12 bytes per pixel cross PCIe.  rgb_hwc: host [h][w][3] u16.  Bit-identical to ssw_writer_create on the
   host-converted frame. */
int ssw_writer_create_rgb16(ssw_ctx* ctx, const uint16_t* rgb_hwc, size_t w, size_t h,
                            const ssw_config* cfg, ssw_writer** out);
/* Writer::coefficient_image(), src/algorithm.rs:319-321 -> host [h][w]. */
int ssw_writer_coefficients(ssw_writer* wr, float* out_plane);
/* Writer::embed(&mut self, marks), src/algorithm.rs:348-352.  marks[m] has lens[m] floats (host).
   The ordering is the one Writer::new fixed from the ORIGINAL coefficients (:314): a second embed()
   (the reference says "call once", but allows it) still ranks the original plane, not the modified one. */
int ssw_writer_embed(ssw_writer* wr, const float* const* marks, const size_t* lens, size_t n_marks);
/* Writer::result(self), src/algorithm.rs:361-379 -> host [h][w][3]; consumes the writer. */
int ssw_writer_result(ssw_writer* wr, float* out_rgb_hwc);
/* Writer::mark(self, marks), src/algorithm.rs:355-358 = embed + result. */
int ssw_writer_mark(ssw_writer* wr, const float* const* marks, const size_t* lens, size_t n_marks,
                    float* out_rgb_hwc);
/* Writer::result(self).into_rgb8() / Writer::mark(self, marks).into_rgb8() (src/algorithm.rs:355-379 followed
   by the caller's `into_rgb8()`, examples/main.rs:271-278, tests/single_simple.rs:28): round(clamp(v,0,1)*255)
   in the epilogue of the last inverse pass -> host [h][w][3] u8.  Works on writers created from f32 or u8. */
int ssw_writer_result_rgb8(ssw_writer* wr, uint8_t* out_rgb_hwc);
int ssw_writer_mark_rgb8(ssw_writer* wr, const float* const* marks, const size_t* lens, size_t n_marks,
                         uint8_t* out_rgb_hwc);
int ssw_writer_destroy(ssw_writer* wr);

/* Reader::base(image, config) when is_base != 0 (src/algorithm.rs:462-464), else
   Reader::derived / ReaderDerived::new (:453-455, :469-471); cfg may be NULL for a derived reader. */
int ssw_reader_create(ssw_ctx* ctx, const float* rgb_hwc, size_t w, size_t h, int is_base,
                      const ssw_config* cfg, ssw_reader** out);
/* The same on an 8-bit image (`into_rgb32f()`, src/algorithm.rs:476, on the device); host [h][w][3] u8. */
int ssw_reader_create_rgb8(ssw_ctx* ctx, const uint8_t* rgb_hwc, size_t w, size_t h, int is_base,
                           const ssw_config* cfg, ssw_reader** out);
/* ... and on a 16-bit image (v / 65535; src/algorithm.rs:476); host [h][w][3] u16. */
int ssw_reader_create_rgb16(ssw_ctx* ctx, const uint16_t* rgb_hwc, size_t w, size_t h, int is_base,
                            const ssw_config* cfg, ssw_reader** out);
/* Reader::coefficients(), src/algorithm.rs:502-504 -> host [h*w]. */
int ssw_reader_coefficients(ssw_reader* rd, float* out_plane);
/* Reader::indices(), src/algorithm.rs:506-508: first k entries (k <= w*h-1) as u64 (`usize`). */
int ssw_reader_indices(ssw_reader* rd, size_t k, uint64_t* out);
/* Reader::extract(&self, &derived, &mut [f32]), src/algorithm.rs:529-539. */
int ssw_reader_extract(ssw_reader* base, ssw_reader* derived, float* out, size_t k);
int ssw_reader_destroy(ssw_reader* rd);

/* Tester::new(extracted).similarity(mark), src/algorithm.rs:689-714 (host buffers, computed on the GPU). */
int ssw_similarity(ssw_ctx* ctx, const float* extracted, size_t n_extracted,
                   const float* mark, size_t n_mark, float* out_similarity);

/* ---- synthetic input (bench / parity plumbing, not in the reference) ------- */
/* Deterministic multi-octave value-noise frames, bit-identical to the oracle's
   generator: frame index = first_frame + i.  dev_rgb: [n_frames][h][w][3]. */
int ssw_synth_frames(ssw_ctx* ctx, uint32_t seed, uint32_t first_frame, size_t n_frames,
                     size_t w, size_t h, float* dev_rgb);

#ifdef __cplusplus
}
#endif
#endif /* SSW_H */
