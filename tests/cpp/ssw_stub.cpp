// ssw_stub.cpp -- a contract stand-in for libssw_hip.so: every extern "C" entry point that include/ssw.hpp names, written by
// hand against the comments of include/ssw.h, with no HIP and no GPU.  tests/cpp/wrappers_stub_test.cpp links it INSTEAD of
// the library (tests/test_cpp_wrappers_cpu.py), so a wrapper that starts calling a new entry point fails the link until its
// contract is stated here.  The C++ counterpart of tests/fake_ssw.py.
//   * "Device" memory is host memory: ssw_dev_alloc / ssw_host_alloc return heap blocks of exactly the bytes asked for, and
//     the stub keeps tables of the live device blocks, pinned blocks, contexts, writers and readers.  Freeing something that
//     is not live aborts with a message.
//   * Every compute entry point READS every byte its contract says it reads (host inputs directly, device inputs after a
//     lookup of the block and a bounds check) into a checksum, and WRITES every byte its contract says it writes, with a
//     pattern that encodes the position (stated at each function), so that a wrapper's slicing can be checked and an
//     undersized buffer is an AddressSanitizer report.
//   * The scalar arguments (and job fields) of the last compute call are kept: ssw_stub_last(i).
//   * ssw_stub_fail_at(n, status): the n-th entry-point call from now answers `status` with no effect.  Exempt, and not
//     counted by ssw_stub_calls(): ssw_status_string, ssw_last_error, every *_destroy, ssw_dev_free, ssw_host_free
//     (destructors cannot report) and ssw_ctx_pass_frames (it has no status to answer with).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <vector>

#include "ssw.h"

struct ssw_ctx { int device; };
struct ssw_writer { ssw_ctx* ctx; size_t w, h; bool consumed; };
struct ssw_reader { ssw_ctx* ctx; size_t w, h; bool is_base; };

namespace {
std::map<const uint8_t*, size_t> g_dev, g_pinned;
std::set<const void*> g_ctx, g_writers, g_readers;
uint64_t g_sum = 0;
size_t g_calls = 0, g_fail_in = 0;
int g_fail_status = SSW_OK;
std::vector<double> g_last;

[[noreturn]] void die(const char* what) {
    std::fprintf(stderr, "ssw_stub: %s\n", what);
    std::abort();
}
void eat(const void* p, size_t bytes) {
    const uint8_t* b = static_cast<const uint8_t*>(p);
    for (size_t i = 0; i < bytes; ++i) g_sum = g_sum * 31 + b[i];
}
template <class T> void eat_n(const T* p, size_t n) { eat(p, n * sizeof(T)); }
void fill(void* p, uint8_t v, size_t bytes) { if (bytes) std::memset(p, v, bytes); }
// the device block that holds [p, p + bytes)
uint8_t* dev(const void* p, size_t bytes) {
    const uint8_t* b = static_cast<const uint8_t*>(p);
    auto it = g_dev.upper_bound(b);
    if (it == g_dev.begin()) die("not a device pointer");
    --it;
    if (b + bytes > it->first + it->second) die("device access beyond the block");
    return const_cast<uint8_t*>(b);
}
void dev_eat(const void* p, size_t bytes) { eat(dev(p, bytes), bytes); }
bool live(ssw_ctx* c) {
    if (c && !g_ctx.count(c)) die("context is not live");
    return c != nullptr;
}
bool live(ssw_writer* w) {
    if (w && !g_writers.count(w)) die("writer is not live");
    return w != nullptr;
}
bool live(ssw_reader* r) {
    if (r && !g_readers.count(r)) die("reader is not live");
    return r != nullptr;
}
template <class... A> void note(A... a) { g_last = {static_cast<double>(a)...}; }
bool finite6(const double* m) {
    for (int i = 0; i < 6; ++i) if (!std::isfinite(m[i])) return false;
    return true;
}
size_t ph_of(size_t sw, size_t sh, size_t pw) { return std::max<size_t>(1, (2 * sh * pw + sw) / (2 * sw)); }
}  // namespace

#define ENTER()                                                        \
    do {                                                               \
        ++g_calls;                                                     \
        if (g_fail_in && --g_fail_in == 0) return g_fail_status;       \
    } while (0)

extern "C" {
// ---- the test's hooks ------------------------------------------------------------------------------------------------------
void ssw_stub_fail_at(size_t n, int status) { g_fail_in = n; g_fail_status = status; }
size_t ssw_stub_calls(void) { return g_calls; }
void ssw_stub_live(size_t out[5]) {
    out[0] = g_dev.size(); out[1] = g_pinned.size(); out[2] = g_ctx.size(); out[3] = g_writers.size(); out[4] = g_readers.size();
}
double ssw_stub_last(size_t i) { return i < g_last.size() ? g_last[i] : -1.0; }
uint64_t ssw_stub_checksum(void) { return g_sum; }

// ---- library / context -----------------------------------------------------------------------------------------------------
const char* ssw_status_string(int status) {
    static const char* const names[] = {"ok", "bad argument", "bad dimensions", "length mismatch", "k too large", "not a base reader",
                                        "unsupported", "consumed", "HIP error", "no device", "out of memory"};
    return status >= 0 && status <= SSW_ERR_OUT_OF_MEMORY ? names[status] : "unknown";
}
const char* ssw_last_error(void) { return "stub"; }
int ssw_ctx_create(int device_id, ssw_ctx** out) {
    ENTER();
    if (!out) return SSW_ERR_BAD_ARG;
    *out = new ssw_ctx{device_id};
    g_ctx.insert(*out);
    note(device_id);
    return SSW_OK;
}
int ssw_ctx_destroy(ssw_ctx* ctx) {
    if (!live(ctx)) return SSW_OK;
    g_ctx.erase(ctx);
    delete ctx;
    return SSW_OK;
}
#define CTX_SETTER(name, type)                       \
    int name(ssw_ctx* ctx, type v) {                 \
        ENTER();                                     \
        if (!live(ctx)) return SSW_ERR_BAD_ARG;      \
        note((double)(uintptr_t)v);                   \
        return SSW_OK;                               \
    }
int ssw_ctx_synchronize(ssw_ctx* ctx) {
    ENTER();
    return live(ctx) ? SSW_OK : SSW_ERR_BAD_ARG;
}
CTX_SETTER(ssw_ctx_set_stream, void*)
CTX_SETTER(ssw_ctx_wait_event, void*)
CTX_SETTER(ssw_ctx_record_event, void*)
CTX_SETTER(ssw_ctx_set_chunk_frames, size_t)
CTX_SETTER(ssw_ctx_set_overlap, int)
CTX_SETTER(ssw_ctx_set_prune, int)
CTX_SETTER(ssw_ctx_set_odd_split, int)
CTX_SETTER(ssw_ctx_set_copy_threads, int)
// no status to answer with: n_frames, w and h come back in one number
size_t ssw_ctx_pass_frames(ssw_ctx* ctx, size_t n_frames, size_t w, size_t h) { return live(ctx) ? n_frames * 1000000 + w * 1000 + h : 0; }
// stats[i] = i + 1
int ssw_ctx_get_transfer_stats(ssw_ctx* ctx, double* stats, int reset) {
    ENTER();
    if (!live(ctx)) return SSW_ERR_BAD_ARG;
    for (int i = 0; stats && i < SSW_TRANSFER_STAT_COUNT; ++i) stats[i] = i + 1;
    note(reset);
    return SSW_OK;
}

// ---- memory ----------------------------------------------------------------------------------------------------------------
static int block_alloc(std::map<const uint8_t*, size_t>& table, size_t bytes, void** out) {
    void* p = std::malloc(bytes);
    if (!p) return SSW_ERR_OUT_OF_MEMORY;
    fill(p, 0xEE, bytes);
    table[static_cast<const uint8_t*>(p)] = bytes;
    *out = p;
    return SSW_OK;
}
static int block_free(std::map<const uint8_t*, size_t>& table, void* p, const char* what) {
    if (!p) return SSW_OK;
    if (!table.erase(static_cast<const uint8_t*>(p))) die(what);
    std::free(p);
    return SSW_OK;
}
int ssw_dev_alloc(ssw_ctx* ctx, size_t bytes, void** dev_ptr) {
    ENTER();
    if (!live(ctx) || !dev_ptr) return SSW_ERR_BAD_ARG;
    return block_alloc(g_dev, bytes, dev_ptr);
}
int ssw_dev_free(ssw_ctx* ctx, void* dev_ptr) {
    if (!live(ctx)) return SSW_ERR_BAD_ARG;
    return block_free(g_dev, dev_ptr, "ssw_dev_free of a block that is not live");
}
int ssw_host_alloc(ssw_ctx* ctx, size_t bytes, void** host_ptr) {
    ENTER();
    if (!live(ctx) || !host_ptr) return SSW_ERR_BAD_ARG;
    return block_alloc(g_pinned, bytes, host_ptr);
}
int ssw_host_free(ssw_ctx* ctx, void* host_ptr) {
    if (!live(ctx)) return SSW_ERR_BAD_ARG;
    return block_free(g_pinned, host_ptr, "ssw_host_free of a block that is not live");
}
int ssw_copy_to_dev(ssw_ctx* ctx, void* dev_dst, const void* host_src, size_t bytes) {
    ENTER();
    if (!live(ctx)) return SSW_ERR_BAD_ARG;
    if (bytes == 0) return SSW_OK;
    if (!dev_dst || !host_src) return SSW_ERR_BAD_ARG;
    eat(host_src, bytes);
    std::memcpy(dev(dev_dst, bytes), host_src, bytes);
    return SSW_OK;
}
int ssw_copy_to_host(ssw_ctx* ctx, void* host_dst, const void* dev_src, size_t bytes) {
    ENTER();
    if (!live(ctx)) return SSW_ERR_BAD_ARG;
    if (bytes == 0) return SSW_OK;
    if (!host_dst || !dev_src) return SSW_ERR_BAD_ARG;
    std::memcpy(host_dst, dev(dev_src, bytes), bytes);
    return SSW_OK;
}

// ---- Writer ----------------------------------------------------------------------------------------------------------------
static int writer_create(ssw_ctx* ctx, const void* rgb, size_t elem, size_t w, size_t h, const ssw_config* cfg, ssw_writer** out) {
    if (!live(ctx) || !rgb || !out) return SSW_ERR_BAD_ARG;
    if (w == 0 || h == 0) return SSW_ERR_BAD_DIMS;
    if (cfg && (cfg->ordering == SSW_ORDER_CUSTOM || cfg->method == SSW_METHOD_CUSTOM)) return SSW_ERR_UNSUPPORTED;
    eat(rgb, w * h * 3 * elem);
    if (cfg) { eat_n(cfg, 1); note(elem, w, h, cfg->ordering, cfg->method, cfg->alpha, cfg->precision); }
    *out = new ssw_writer{ctx, w, h, false};
    g_writers.insert(*out);
    return SSW_OK;
}
int ssw_writer_create(ssw_ctx* ctx, const float* rgb, size_t w, size_t h, const ssw_config* cfg, ssw_writer** out) {
    ENTER();
    return writer_create(ctx, rgb, 4, w, h, cfg, out);
}
int ssw_writer_create_rgb8(ssw_ctx* ctx, const uint8_t* rgb, size_t w, size_t h, const ssw_config* cfg, ssw_writer** out) {
    ENTER();
    return writer_create(ctx, rgb, 1, w, h, cfg, out);
}
int ssw_writer_create_rgb16(ssw_ctx* ctx, const uint16_t* rgb, size_t w, size_t h, const ssw_config* cfg, ssw_writer** out) {
    ENTER();
    return writer_create(ctx, rgb, 2, w, h, cfg, out);
}
int ssw_writer_destroy(ssw_writer* wr) {
    if (!live(wr)) return SSW_OK;
    g_writers.erase(wr);
    delete wr;
    return SSW_OK;
}
// out[j] = j
int ssw_writer_coefficients(ssw_writer* wr, float* out_plane) {
    ENTER();
    if (!live(wr) || !out_plane) return SSW_ERR_BAD_ARG;
    for (size_t j = 0; j < wr->w * wr->h; ++j) out_plane[j] = (float)j;
    return SSW_OK;
}
int ssw_writer_embed(ssw_writer* wr, const float* const* marks, const size_t* lens, size_t n_marks) {
    ENTER();
    if (!live(wr) || (n_marks && (!marks || !lens))) return SSW_ERR_BAD_ARG;
    if (wr->consumed) return SSW_ERR_CONSUMED;
    eat_n(marks, n_marks);
    eat_n(lens, n_marks);
    for (size_t m = 0; m < n_marks; ++m) {
        if (!marks[m]) return SSW_ERR_BAD_ARG;
        eat_n(marks[m], lens[m]);
    }
    note(n_marks, n_marks ? lens[0] : 0);
    return SSW_OK;
}
// the one frame is frame 0: every byte 1
int ssw_writer_result(ssw_writer* wr, float* out) {
    ENTER();
    if (!live(wr) || !out) return SSW_ERR_BAD_ARG;
    if (wr->consumed) return SSW_ERR_CONSUMED;
    fill(out, 1, wr->w * wr->h * 3 * sizeof(float));
    wr->consumed = true;
    return SSW_OK;
}
int ssw_writer_result_rgb8(ssw_writer* wr, uint8_t* out) {
    ENTER();
    if (!live(wr) || !out) return SSW_ERR_BAD_ARG;
    if (wr->consumed) return SSW_ERR_CONSUMED;
    fill(out, 1, wr->w * wr->h * 3);
    wr->consumed = true;
    return SSW_OK;
}
// copy i is filled with the value i + 1
extern "C++" {
template <class T> static int mark_copies(ssw_writer* wr, const float* marks, size_t n, size_t k, T* out) {
    if (!live(wr) || (n && (!marks || !out))) return SSW_ERR_BAD_ARG;
    if (wr->consumed) return SSW_ERR_CONSUMED;
    eat_n(marks, n * k);
    const size_t f = wr->w * wr->h * 3;
    for (size_t i = 0; i < n; ++i)
        for (size_t j = 0; j < f; ++j) out[i * f + j] = (T)(i + 1);
    note(n, k);
    return SSW_OK;
}
}
int ssw_writer_mark_copies(ssw_writer* wr, const float* marks, size_t n, size_t k, float* out) {
    ENTER();
    return mark_copies(wr, marks, n, k, out);
}
int ssw_writer_mark_copies_rgb8(ssw_writer* wr, const float* marks, size_t n, size_t k, uint8_t* out) {
    ENTER();
    return mark_copies(wr, marks, n, k, out);
}

// ---- Reader ----------------------------------------------------------------------------------------------------------------
static int reader_create(ssw_ctx* ctx, const void* rgb, size_t elem, size_t w, size_t h, int is_base, const ssw_config* cfg, ssw_reader** out) {
    if (!live(ctx) || !rgb || !out || (is_base && !cfg)) return SSW_ERR_BAD_ARG;
    if (w == 0 || h == 0) return SSW_ERR_BAD_DIMS;
    if (cfg && (cfg->ordering == SSW_ORDER_CUSTOM || cfg->method == SSW_METHOD_CUSTOM)) return SSW_ERR_UNSUPPORTED;
    eat(rgb, w * h * 3 * elem);
    if (cfg) { eat_n(cfg, 1); note(elem, w, h, cfg->ordering, cfg->method, cfg->alpha, cfg->precision, is_base); }
    *out = new ssw_reader{ctx, w, h, is_base != 0};
    g_readers.insert(*out);
    return SSW_OK;
}
int ssw_reader_create(ssw_ctx* ctx, const float* rgb, size_t w, size_t h, int is_base, const ssw_config* cfg, ssw_reader** out) {
    ENTER();
    return reader_create(ctx, rgb, 4, w, h, is_base, cfg, out);
}
int ssw_reader_create_rgb8(ssw_ctx* ctx, const uint8_t* rgb, size_t w, size_t h, int is_base, const ssw_config* cfg, ssw_reader** out) {
    ENTER();
    return reader_create(ctx, rgb, 1, w, h, is_base, cfg, out);
}
int ssw_reader_create_rgb16(ssw_ctx* ctx, const uint16_t* rgb, size_t w, size_t h, int is_base, const ssw_config* cfg, ssw_reader** out) {
    ENTER();
    return reader_create(ctx, rgb, 2, w, h, is_base, cfg, out);
}
int ssw_reader_destroy(ssw_reader* rd) {
    if (!live(rd)) return SSW_OK;
    g_readers.erase(rd);
    delete rd;
    return SSW_OK;
}
// out[j] = j
int ssw_reader_coefficients(ssw_reader* rd, float* out_plane) {
    ENTER();
    if (!live(rd) || !out_plane) return SSW_ERR_BAD_ARG;
    for (size_t j = 0; j < rd->w * rd->h; ++j) out_plane[j] = (float)j;
    return SSW_OK;
}
// out[j] = j
int ssw_reader_indices(ssw_reader* rd, size_t k, uint64_t* out) {
    ENTER();
    if (!live(rd) || (k && !out)) return SSW_ERR_BAD_ARG;
    if (!rd->is_base) return SSW_ERR_NOT_BASE;
    if (k > rd->w * rd->h - 1) return SSW_ERR_K_TOO_LARGE;
    for (size_t j = 0; j < k; ++j) out[j] = j;
    return SSW_OK;
}
// out[j] = j + 0.5
int ssw_reader_extract(ssw_reader* base, ssw_reader* derived, float* out, size_t k) {
    ENTER();
    if (!live(base) || !live(derived) || (k && !out)) return SSW_ERR_BAD_ARG;
    if (!base->is_base) return SSW_ERR_NOT_BASE;
    if (base->w * base->h != derived->w * derived->h) return SSW_ERR_LENGTH_MISMATCH;
    if (k >= base->w * base->h) return SSW_ERR_K_TOO_LARGE;
    for (size_t j = 0; j < k; ++j) out[j] = (float)j + 0.5f;
    return SSW_OK;
}
// ext[s][j] = 1000 s + j, sims[s][m] = 100 s + m, best[s] = s, best_sim[s] = s + 0.5, n_exceed[s] = s + 2
static int trace_out(size_t plane, size_t n, size_t k, const float* marks, size_t nm, float threshold, float* ext, float* sims, uint32_t* best,
                     float* best_sim, uint32_t* n_exceed) {
    if (!marks && (nm || sims || best || best_sim || n_exceed)) return SSW_ERR_BAD_ARG;
    if (k >= plane) return SSW_ERR_K_TOO_LARGE;
    eat_n(marks, nm * k);
    for (size_t s = 0; s < n; ++s) {
        for (size_t j = 0; ext && j < k; ++j) ext[s * k + j] = (float)(1000 * s + j);
        for (size_t m = 0; sims && m < nm; ++m) sims[s * nm + m] = (float)(100 * s + m);
        if (best) best[s] = (uint32_t)s;
        if (best_sim) best_sim[s] = (float)s + 0.5f;
        if (n_exceed) n_exceed[s] = (uint32_t)s + 2;
    }
    note(n, k, nm, threshold);
    return SSW_OK;
}
int ssw_reader_trace_host_rgb8(ssw_reader* base, const uint8_t* const* suspects, size_t n, size_t k, const float* marks, size_t nm,
                               float threshold, float* ext, float* sims, uint32_t* best, float* best_sim, uint32_t* n_exceed) {
    ENTER();
    if (!live(base) || (n && !suspects)) return SSW_ERR_BAD_ARG;
    if (!base->is_base) return SSW_ERR_NOT_BASE;
    eat_n(suspects, n);
    for (size_t s = 0; s < n; ++s) {
        if (!suspects[s]) return SSW_ERR_BAD_ARG;
        eat(suspects[s], base->w * base->h * 3);
    }
    return trace_out(base->w * base->h, n, k, marks, nm, threshold, ext, sims, best, best_sim, n_exceed);
}
static bool placement_ok(const ssw_placement& p, size_t W, size_t H) {
    const size_t pw = p.pw ? p.pw : p.w, ph = p.ph ? p.ph : p.h;
    return (p.channels == 3 || p.channels == 4) && p.w && p.h && (p.pw != 0) == (p.ph != 0) && p.x + pw <= W && p.y + ph <= H;
}
// the outputs of ssw_reader_trace_host_rgb8; ssw_stub_last(4 + 7 s ...) = the fields of placement s
int ssw_reader_trace_restored_host_rgb8(ssw_reader* base, const uint8_t* base_rgb, const uint8_t* const* suspects, const ssw_placement* pl,
                                        size_t n, size_t k, const float* marks, size_t nm, float threshold, float* ext, float* sims,
                                        uint32_t* best, float* best_sim, uint32_t* n_exceed) {
    ENTER();
    if (!live(base) || (n && (!suspects || !pl))) return SSW_ERR_BAD_ARG;
    if (!base->is_base) return SSW_ERR_NOT_BASE;
    eat_n(suspects, n);
    eat_n(pl, n);
    bool reads_base = false;
    for (size_t s = 0; s < n; ++s) {
        if (!suspects[s] || !placement_ok(pl[s], base->w, base->h)) return SSW_ERR_BAD_ARG;
        eat(suspects[s], (size_t)pl[s].w * pl[s].h * pl[s].channels);
        const size_t pw = pl[s].pw ? pl[s].pw : pl[s].w, ph = pl[s].ph ? pl[s].ph : pl[s].h;
        reads_base = reads_base || pl[s].channels == 4 || pw != base->w || ph != base->h;
    }
    if (reads_base && !base_rgb) return SSW_ERR_BAD_ARG;
    if (base_rgb) eat(base_rgb, base->w * base->h * 3);
    const int rc = trace_out(base->w * base->h, n, k, marks, nm, threshold, ext, sims, best, best_sim, n_exceed);
    for (size_t s = 0; s < n; ++s)
        for (uint32_t v : {pl[s].w, pl[s].h, pl[s].channels, pl[s].x, pl[s].y, pl[s].pw, pl[s].ph}) g_last.push_back(v);
    return rc;
}
// out = extracted count + 0.25
int ssw_similarity(ssw_ctx* ctx, const float* extracted, size_t n_extracted, const float* mark, size_t n_mark, float* out) {
    ENTER();
    if (!live(ctx) || !extracted || !mark || !out) return SSW_ERR_BAD_ARG;
    if (n_extracted != n_mark) return SSW_ERR_LENGTH_MISMATCH;
    eat_n(extracted, n_extracted);
    eat_n(mark, n_mark);
    *out = (float)n_extracted + 0.25f;
    return SSW_OK;
}

// ---- locate, signatures ----------------------------------------------------------------------------------------------------
static int locate_in(ssw_ctx* ctx, const uint8_t* dev_base, size_t w, size_t h, const void* const* dev_suspects, const ssw_placement* pl, size_t n,
                     const uint64_t* sad) {
    if (!live(ctx) || !dev_base || !dev_suspects || !pl || !sad) return SSW_ERR_BAD_ARG;
    if (w == 0 || h == 0) return SSW_ERR_BAD_ARG;
    dev_eat(dev_base, w * h * 3);
    eat_n(dev_suspects, n);
    eat_n(pl, n);
    for (size_t i = 0; i < n; ++i) {
        if (!dev_suspects[i] || (pl[i].channels != 3 && pl[i].channels != 4) || !pl[i].w || !pl[i].h) return SSW_ERR_BAD_ARG;
        dev_eat(dev_suspects[i], (size_t)pl[i].w * pl[i].h * pl[i].channels);
    }
    return SSW_OK;
}
// x = 10 + i, y = 20 + i, sad[i] = 1000 + i
int ssw_locate_rgb8(ssw_ctx* ctx, const uint8_t* dev_base, size_t w, size_t h, const void* const* dev_suspects, ssw_placement* pl, size_t n,
                    uint64_t* sad) {
    ENTER();
    if (live(ctx) && n == 0) return SSW_OK;
    const int rc = locate_in(ctx, dev_base, w, h, dev_suspects, pl, n, sad);
    if (rc != SSW_OK) return rc;
    for (size_t i = 0; i < n; ++i) {
        const size_t pw = pl[i].pw ? pl[i].pw : pl[i].w, ph = pl[i].ph ? pl[i].ph : pl[i].h;
        if ((pl[i].pw != 0) != (pl[i].ph != 0) || pw > w || ph > h) return SSW_ERR_BAD_ARG;
    }
    for (size_t i = 0; i < n; ++i) { pl[i].x = 10 + (uint32_t)i; pl[i].y = 20 + (uint32_t)i; sad[i] = 1000 + i; }
    note(w, h, n);
    return SSW_OK;
}
// ... and pw = 64 + 8 i, ph = ph(pw) of the aspect ratio
int ssw_locate_scaled_rgb8(ssw_ctx* ctx, const uint8_t* dev_base, size_t w, size_t h, const void* const* dev_suspects, ssw_placement* pl,
                           const ssw_scale_range* ranges, size_t n, uint64_t* sad) {
    ENTER();
    if (live(ctx) && n == 0) return SSW_OK;
    if (!ranges) return SSW_ERR_BAD_ARG;
    const int rc = locate_in(ctx, dev_base, w, h, dev_suspects, pl, n, sad);
    if (rc != SSW_OK) return rc;
    eat_n(ranges, n);
    for (size_t i = 0; i < n; ++i) {
        const size_t wmin = ranges[i].wmin, phmin = ph_of(pl[i].w, pl[i].h, wmin);
        if (wmin > ranges[i].wmax || std::min(wmin, phmin) < 32 || wmin > w || phmin > h) return SSW_ERR_BAD_ARG;
    }
    note(w, h, n);
    for (size_t i = 0; i < n; ++i) {
        pl[i].pw = 64 + 8 * (uint32_t)i; pl[i].ph = (uint32_t)ph_of(pl[i].w, pl[i].h, pl[i].pw);
        pl[i].x = 10 + (uint32_t)i; pl[i].y = 20 + (uint32_t)i; sad[i] = 1000 + i;
        g_last.push_back(ranges[i].wmin); g_last.push_back(ranges[i].wmax);
    }
    return SSW_OK;
}
// signature i is filled with i + 1
int ssw_signature_host_rgb8(ssw_ctx* ctx, const uint8_t* const* frames, const ssw_image_shape* shapes, size_t n, uint8_t* sigs) {
    ENTER();
    if (!live(ctx)) return SSW_ERR_BAD_ARG;
    if (n == 0) return SSW_OK;
    if (!frames || !shapes || !sigs) return SSW_ERR_BAD_ARG;
    eat_n(frames, n);
    eat_n(shapes, n);
    for (size_t i = 0; i < n; ++i) {
        if (!frames[i] || shapes[i].w < 32 || shapes[i].h < 32 || (shapes[i].channels != 3 && shapes[i].channels != 4)) return SSW_ERR_BAD_ARG;
        eat(frames[i], (size_t)shapes[i].w * shapes[i].h * shapes[i].channels);
    }
    for (size_t i = 0; i < n; ++i) fill(sigs + i * 1024, (uint8_t)(i + 1), 1024);
    return SSW_OK;
}
// index[s][t] = 8 s + t, distance[s][t] = 100 s + t; both 0xFFFFFFFF from t = nc on
int ssw_signature_match(ssw_ctx* ctx, const uint8_t* dev_query, size_t nq, const uint8_t* dev_catalogue, size_t nc, size_t top,
                        uint32_t* dev_index, uint32_t* dev_dist, uint32_t* dev_all) {
    ENTER();
    if (!live(ctx) || top < 1 || top > 8 || nc > 0xFFFFFFFFull) return SSW_ERR_BAD_ARG;
    if (nq == 0) return SSW_OK;
    if (!dev_query || !dev_index || !dev_dist || (nc && !dev_catalogue)) return SSW_ERR_BAD_ARG;
    dev_eat(dev_query, nq * 1024);
    if (nc) dev_eat(dev_catalogue, nc * 1024);
    uint32_t* index = reinterpret_cast<uint32_t*>(dev(dev_index, nq * top * 4));
    uint32_t* dist = reinterpret_cast<uint32_t*>(dev(dev_dist, nq * top * 4));
    for (size_t s = 0; s < nq; ++s)
        for (size_t t = 0; t < top; ++t) {
            index[s * top + t] = t < nc ? (uint32_t)(8 * s + t) : 0xFFFFFFFFu;
            dist[s * top + t] = t < nc ? (uint32_t)(100 * s + t) : 0xFFFFFFFFu;
        }
    if (dev_all) fill(dev(dev_all, nq * nc * 4), 7, nq * nc * 4);
    note(nq, nc, top);
    return SSW_OK;
}

// ---- the strength report: statistics -------------------------------------------------------------------------------------------
// word j of copy i = 16 i + j
static int against(ssw_ctx* ctx, const uint8_t* dev_base, size_t n_base, const uint8_t* dev_copies, size_t n, size_t w, size_t h, uint64_t* dev_stats,
                   size_t words, size_t min_side) {
    if (!live(ctx)) return SSW_ERR_BAD_ARG;
    if (n == 0) return SSW_OK;
    if (!dev_base || !dev_copies || !dev_stats || (n_base != 1 && n_base != n) || (w && h && (w < min_side || h < min_side))) return SSW_ERR_BAD_ARG;
    if (w == 0 || h == 0) return SSW_ERR_BAD_DIMS;
    dev_eat(dev_base, n_base * w * h * 3);
    dev_eat(dev_copies, n * w * h * 3);
    uint64_t* st = reinterpret_cast<uint64_t*>(dev(dev_stats, n * words * 8));
    for (size_t i = 0; i < n; ++i)
        for (size_t j = 0; j < words; ++j) st[i * words + j] = 16 * i + j;
    note(n_base, n, w, h);
    return SSW_OK;
}
int ssw_quality_rgb8(ssw_ctx* ctx, const uint8_t* dev_base, size_t n_base, const uint8_t* dev_copies, size_t n, size_t w, size_t h, uint64_t* dev_stats) {
    ENTER();
    return against(ctx, dev_base, n_base, dev_copies, n, w, h, dev_stats, 6, 1);
}
int ssw_ssim_rgb8(ssw_ctx* ctx, const uint8_t* dev_base, size_t n_base, const uint8_t* dev_copies, size_t n, size_t w, size_t h, uint64_t* dev_stats,
                  int32_t* dev_map) {
    ENTER();
    const int rc = against(ctx, dev_base, n_base, dev_copies, n, w, h, dev_stats, SSW_SSIM_STATS, SSW_SSIM_MIN_SIDE);
    if (rc == SSW_OK && n && dev_map) fill(dev(dev_map, n * (w / 4 - 1) * (h / 4 - 1) * 4), 3, n * (w / 4 - 1) * (h / 4 - 1) * 4);
    return rc;
}

// ---- the strength report: frame-producing calls; output frame j is filled with the byte (j + 1) & 255 -----------------------------
static void frames_out(uint8_t* dev_out, size_t m, size_t frame_bytes) {
    uint8_t* out = dev(dev_out, m * frame_bytes);
    for (size_t j = 0; j < m; ++j) fill(out + j * frame_bytes, (uint8_t)((j + 1) & 255), frame_bytes);
}
// the frames and the job array are read; ok(job) is the header's own argument check
extern "C++" {
template <class Job, class Ok>
static int through_jobs(ssw_ctx* ctx, const uint8_t* dev_frames, size_t n, size_t w, size_t h, const Job* jobs, size_t m, uint8_t* dev_out, size_t min_side,
                        Ok ok) {
    if (!live(ctx)) return SSW_ERR_BAD_ARG;
    if (m == 0) return SSW_OK;
    if (!dev_frames || !jobs || !dev_out) return SSW_ERR_BAD_ARG;
    if (w == 0 || h == 0 || w > 65535 || h > 65535) return SSW_ERR_BAD_DIMS;
    if (w < min_side || h < min_side) return SSW_ERR_BAD_ARG;
    eat_n(jobs, m);
    for (size_t j = 0; j < m; ++j) if (!ok(jobs[j])) return SSW_ERR_BAD_ARG;
    dev_eat(dev_frames, n * w * h * 3);
    frames_out(dev_out, m, w * h * 3);
    return SSW_OK;
}
}
int ssw_collude_rgb8(ssw_ctx* ctx, const uint8_t* dev_copies, size_t n, size_t w, size_t h, const ssw_coalition* co, size_t m, uint8_t* dev_out) {
    ENTER();
    const int rc = through_jobs(ctx, dev_copies, n, w, h, co, m, dev_out, 1, [&](const ssw_coalition& c) {
        if (c.method > SSW_COLLUDE_MOSAIC || c.count < 1 || c.count > 16) return false;
        for (uint32_t i = 0; i < c.count; ++i) if (c.member[i] >= n) return false;
        return true;
    });
    if (rc == SSW_OK && m) note(n, w, h, m, co[m - 1].method, co[m - 1].count, co[m - 1].member[co[m - 1].count - 1]);
    return rc;
}
int ssw_jpeg_rgb8(ssw_ctx* ctx, const uint8_t* dev_frames, size_t n, size_t w, size_t h, const ssw_jpeg_job* jobs, size_t m, uint8_t* dev_out) {
    ENTER();
    const int rc = through_jobs(ctx, dev_frames, n, w, h, jobs, m, dev_out, 8,
                                [&](const ssw_jpeg_job& j) { return j.frame < n && j.quality >= 1 && j.quality <= 100; });
    if (rc == SSW_OK && m) note(n, w, h, m, jobs[m - 1].frame, jobs[m - 1].quality);
    return rc;
}
int ssw_filter_rgb8(ssw_ctx* ctx, const uint8_t* dev_frames, size_t n, size_t w, size_t h, const ssw_filter_job* jobs, size_t m, uint8_t* dev_out) {
    ENTER();
    const int rc = through_jobs(ctx, dev_frames, n, w, h, jobs, m, dev_out, 1, [&](const ssw_filter_job& j) {
        if (j.frame >= n || j.kind > SSW_FILTER_MEDIAN3) return false;
        const bool radius = j.kind != SSW_FILTER_MEDIAN3, unsharp = j.kind == SSW_FILTER_UNSHARP;
        if (radius ? !(j.radius > 0.0f && j.radius <= 8.0f) : j.radius != 0.0f) return false;
        return unsharp ? j.percent >= 1 && j.percent <= 1000 && j.threshold <= 255 : j.percent == 0 && j.threshold == 0;
    });
    if (rc == SSW_OK && m) note(n, w, h, m, jobs[m - 1].frame, jobs[m - 1].kind, jobs[m - 1].radius, jobs[m - 1].percent, jobs[m - 1].threshold);
    return rc;
}
int ssw_scale_attack_rgb8(ssw_ctx* ctx, const uint8_t* dev_frames, size_t n, size_t w, size_t h, const ssw_scale_job* jobs, size_t m, uint8_t* dev_out) {
    ENTER();
    const int rc = through_jobs(ctx, dev_frames, n, w, h, jobs, m, dev_out, 1, [&](const ssw_scale_job& j) {
        return j.frame < n && j.filter <= SSW_RESAMPLE_LANCZOS && j.nw >= 1 && j.nh >= 1 && j.nw <= 65535 && j.nh <= 65535;
    });
    if (rc == SSW_OK && m) note(n, w, h, m, jobs[m - 1].frame, jobs[m - 1].nw, jobs[m - 1].nh, jobs[m - 1].filter);
    return rc;
}
int ssw_resample_rgb8(ssw_ctx* ctx, const uint8_t* dev_in, size_t n, size_t w, size_t h, size_t nw, size_t nh, int filter, uint8_t* dev_out) {
    ENTER();
    if (!live(ctx)) return SSW_ERR_BAD_ARG;
    if (n == 0) return SSW_OK;
    if (!dev_in || !dev_out || filter < SSW_RESAMPLE_BOX || filter > SSW_RESAMPLE_LANCZOS) return SSW_ERR_BAD_ARG;
    if (!w || !h || !nw || !nh || w > 65535 || h > 65535 || nw > 65535 || nh > 65535) return SSW_ERR_BAD_DIMS;
    dev_eat(dev_in, n * w * h * 3);
    frames_out(dev_out, n, nw * nh * 3);
    note(n, w, h, nw, nh, filter);
    return SSW_OK;
}
// m = {angle, w, h, 3, 4, 5}
int ssw_rotation_matrix(double angle, size_t w, size_t h, double* m) {
    ENTER();
    if (!m || !std::isfinite(angle)) return SSW_ERR_BAD_ARG;
    m[0] = angle; m[1] = (double)w; m[2] = (double)h; m[3] = 3; m[4] = 4; m[5] = 5;
    return SSW_OK;
}
int ssw_affine_rgb8(ssw_ctx* ctx, const uint8_t* dev_in, size_t n, size_t w, size_t h, size_t ow, size_t oh, const double* m, int filter,
                    const uint8_t* fill3, uint8_t* dev_out) {
    ENTER();
    if (!live(ctx)) return SSW_ERR_BAD_ARG;
    if (n == 0) return SSW_OK;
    if (!dev_in || !dev_out || !m || !fill3 || (filter != SSW_AFFINE_BILINEAR && filter != SSW_AFFINE_BICUBIC) || !finite6(m)) return SSW_ERR_BAD_ARG;
    if (!w || !h || !ow || !oh || w > 65535 || h > 65535 || ow > 65535 || oh > 65535) return SSW_ERR_BAD_DIMS;
    eat_n(m, 6);
    eat_n(fill3, 3);
    dev_eat(dev_in, n * w * h * 3);
    frames_out(dev_out, n, ow * oh * 3);
    note(n, w, h, ow, oh, filter, fill3[0], fill3[1], fill3[2], m[0], m[1], m[2], m[3], m[4], m[5]);
    return SSW_OK;
}
static bool rotate_job_ok(const ssw_rotate_job& j, size_t n) {
    return j.frame < n && (j.filter == SSW_AFFINE_BILINEAR || j.filter == SSW_AFFINE_BICUBIC) && finite6(j.forward) && finite6(j.back);
}
static void note_rotate(size_t n, size_t w, size_t h, size_t m, const ssw_rotate_job& j) {
    note(n, w, h, m, j.frame, j.filter, j.fill[0], j.fill[1], j.fill[2], j.forward[0], j.forward[1], j.forward[2], j.back[0], j.back[1], j.back[2]);
}
int ssw_rotate_attack_rgb8(ssw_ctx* ctx, const uint8_t* dev_base, const uint8_t* dev_frames, size_t n, size_t w, size_t h, const ssw_rotate_job* jobs,
                           size_t m, uint8_t* dev_out) {
    ENTER();
    if (live(ctx) && m && !dev_base) return SSW_ERR_BAD_ARG;
    const int rc = through_jobs(ctx, dev_frames, n, w, h, jobs, m, dev_out, 1, [&](const ssw_rotate_job& j) { return rotate_job_ok(j, n); });
    if (rc == SSW_OK && m) { dev_eat(dev_base, w * h * 3); note_rotate(n, w, h, m, jobs[m - 1]); }
    return rc;
}
int ssw_unrotate_rgb8(ssw_ctx* ctx, const uint8_t* dev_base, const uint8_t* dev_suspects, size_t n, size_t w, size_t h, const ssw_rotate_job* jobs,
                      uint8_t* dev_out) {
    ENTER();
    if (live(ctx) && n && !dev_base) return SSW_ERR_BAD_ARG;
    const int rc = through_jobs(ctx, dev_suspects, n, w, h, jobs, n, dev_out, 1, [&](const ssw_rotate_job& j) { return rotate_job_ok(j, n); });
    if (rc == SSW_OK && n) { dev_eat(dev_base, w * h * 3); note_rotate(n, w, h, n, jobs[n - 1]); }
    return rc;
}

// ---- host-image streaming ----------------------------------------------------------------------------------------------------
static int host_frames_in(const uint8_t* const* frames, size_t n, size_t w, size_t h) {
    eat_n(frames, n);
    for (size_t i = 0; i < n; ++i) {
        if (!frames[i]) return SSW_ERR_BAD_ARG;
        eat(frames[i], w * h * 3);
    }
    return SSW_OK;
}
// output frame j is filled with the byte j + 1
int ssw_batch_embed_host_rgb8(ssw_ctx* ctx, const ssw_config* cfg, const uint8_t* const* frames, size_t n, size_t w, size_t h, const float* marks, size_t k,
                              uint8_t* const* out) {
    ENTER();
    if (!live(ctx) || !cfg) return SSW_ERR_BAD_ARG;
    if (n == 0) return SSW_OK;
    if (!frames || !marks || !out) return SSW_ERR_BAD_ARG;
    if (w == 0 || h == 0) return SSW_ERR_BAD_DIMS;
    eat_n(cfg, 1);
    const int rc = host_frames_in(frames, n, w, h);
    if (rc != SSW_OK) return rc;
    eat_n(marks, n * k);
    eat_n(out, n);
    for (size_t j = 0; j < n; ++j) {
        if (!out[j]) return SSW_ERR_BAD_ARG;
        fill(out[j], (uint8_t)(j + 1), w * h * 3);
    }
    note(n, w, h, k, cfg->ordering, cfg->method, cfg->alpha, cfg->precision);
    return SSW_OK;
}
// ext[i][j] = 1000 i + j, sims[i] = i + 0.5
int ssw_batch_extract_host_rgb8(ssw_ctx* ctx, const ssw_config* cfg, const uint8_t* const* base, const uint8_t* const* derived, size_t n, size_t w,
                                size_t h, size_t k, float* ext, const float* marks, float* sims) {
    ENTER();
    if (!live(ctx) || !cfg || (marks == nullptr) != (sims == nullptr)) return SSW_ERR_BAD_ARG;
    if (n == 0) return SSW_OK;
    if (!base || !derived || !ext) return SSW_ERR_BAD_ARG;
    if (w == 0 || h == 0) return SSW_ERR_BAD_DIMS;
    if (k >= w * h) return SSW_ERR_K_TOO_LARGE;
    eat_n(cfg, 1);
    int rc = host_frames_in(base, n, w, h);
    if (rc == SSW_OK) rc = host_frames_in(derived, n, w, h);
    if (rc != SSW_OK) return rc;
    if (marks) eat_n(marks, n * k);
    for (size_t i = 0; i < n; ++i) {
        for (size_t j = 0; j < k; ++j) ext[i * k + j] = (float)(1000 * i + j);
        if (sims) sims[i] = (float)i + 0.5f;
    }
    note(n, w, h, k, cfg->ordering, cfg->method, cfg->alpha, cfg->precision);
    return SSW_OK;
}
}  // extern "C"
