// ssw.hpp -- C++17 host-side mirror of the crate's public surface over the C ABI (ssw.h).
//
// The reference is compiled code (Rust); no Rust toolchain exists in this image, so the host side
// above the C ABI is written in C++ with the reference's names, argument meaning and error
// behaviour (file:line relative to the reference tree):
//
//   wm::Writer / WriteConfig / Insertion      src/algorithm.rs:68-112, :285-433
//   wm::Reader / ReaderDerived / ReadConfig    src/algorithm.rs:114-140, :435-594
//   wm::OrderingMethod                         src/algorithm.rs:142-191
//   wm::MarkBuf                                src/algorithm.rs:596-666
//   wm::Tester / Similarity                    src/algorithm.rs:668-715
//
// Where the reference panics, wm::Error (carrying the ssw_status) is thrown.  Images are
// interleaved RGB f32 buffers [h][w][3] -- what `DynamicImage::into_rgb32f()` yields (:308, :476).
// Header-only; link against libssw_hip.so.
#pragma once

#include <algorithm>
#include <array>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>
#include <memory>
#include <random>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "ssw.h"

namespace wm {

class Error : public std::runtime_error {
public:
    Error(int status, const std::string& where)
        : std::runtime_error(where + ": " + ssw_status_string(status) +
                             (status == SSW_ERR_HIP || status == SSW_ERR_OUT_OF_MEMORY ? std::string(" [") + ssw_last_error() + "]" : std::string())),
          status_(status) {}
    int status() const { return status_; }

private:
    int status_;
};

inline void check(int status, const char* where) {
    if (status != SSW_OK) throw Error(status, where);
}

// One per GPU; not thread-safe (the reference's Writer/Reader are !Send).
class Context {
public:
    explicit Context(int device_id = 0) { check(ssw_ctx_create(device_id, &ctx_), "ssw_ctx_create"); }
    ~Context() { ssw_ctx_destroy(ctx_); }
    Context(const Context&) = delete;
    Context& operator=(const Context&) = delete;
    ssw_ctx* get() const { return ctx_; }
    void synchronize() { check(ssw_ctx_synchronize(ctx_), "ssw_ctx_synchronize"); }
    // Stream hand-off for hosts that drive the device-pointer entry points (see the stream contract in ssw.h):
    // hipStream_t / hipEvent_t as opaque pointers, so that this header needs no HIP headers.
    void set_stream(void* hip_stream) { check(ssw_ctx_set_stream(ctx_, hip_stream), "ssw_ctx_set_stream"); }
    void wait_event(void* hip_event) { check(ssw_ctx_wait_event(ctx_, hip_event), "ssw_ctx_wait_event"); }
    void record_event(void* hip_event) { check(ssw_ctx_record_event(ctx_, hip_event), "ssw_ctx_record_event"); }
    // Batch entry points: frames per internal pass (0 = automatic), two passes in flight, pruned derived transform.
    void set_chunk_frames(size_t n) { check(ssw_ctx_set_chunk_frames(ctx_, n), "ssw_ctx_set_chunk_frames"); }
    size_t pass_frames(size_t n_frames, size_t w, size_t h) const { return ssw_ctx_pass_frames(ctx_, n_frames, w, h); }
    void set_overlap(bool on) { check(ssw_ctx_set_overlap(ctx_, on ? 1 : 0), "ssw_ctx_set_overlap"); }
    void set_prune(bool on) { check(ssw_ctx_set_prune(ctx_, on ? 1 : 0), "ssw_ctx_set_prune"); }
    void set_odd_split(bool on) { check(ssw_ctx_set_odd_split(ctx_, on ? 1 : 0), "ssw_ctx_set_odd_split"); }
    // Host-buffer entry points: copy threads of the pinned staging ring (0 = automatic) and the transfer counters.
    void set_copy_threads(int n) { check(ssw_ctx_set_copy_threads(ctx_, n), "ssw_ctx_set_copy_threads"); }
    std::vector<double> transfer_stats(bool reset = false) {
        std::vector<double> st(SSW_TRANSFER_STAT_COUNT);
        check(ssw_ctx_get_transfer_stats(ctx_, st.data(), reset ? 1 : 0), "ssw_ctx_get_transfer_stats");
        return st;
    }

private:
    ssw_ctx* ctx_ = nullptr;
};

// Pinned (page-locked) host memory from the context: an image decoded into it is the DMA source / target of the
// handles, no staging copy (include/ssw.h: ssw_host_alloc).
class PinnedBuffer {
public:
    PinnedBuffer(Context& ctx, size_t bytes) : ctx_(ctx.get()), bytes_(bytes) { check(ssw_host_alloc(ctx_, bytes, &p_), "ssw_host_alloc"); }
    ~PinnedBuffer() { ssw_host_free(ctx_, p_); }
    PinnedBuffer(const PinnedBuffer&) = delete;
    PinnedBuffer& operator=(const PinnedBuffer&) = delete;
    void* data() { return p_; }
    size_t size() const { return bytes_; }

private:
    ssw_ctx* ctx_;
    void* p_ = nullptr;
    size_t bytes_;
};

// Insertion / Extraction (algorithm.rs:68-77, :115-124).  Custom(closure) exists in the reference;
// it cannot cross to the device and yields SSW_ERR_UNSUPPORTED.
struct Insertion {
    int method;
    float alpha;
    static Insertion Option1(float a) { return {SSW_OPTION1, a}; }
    static Insertion Option2(float a) { return {SSW_OPTION2, a}; }
    static Insertion Option3(float a) { return {SSW_OPTION3, a}; }
    static Insertion Custom() { return {SSW_METHOD_CUSTOM, 0.f}; }
};
using Extraction = Insertion;

enum class OrderingMethod : int {
    Energy = SSW_ORDER_ENERGY,
    EnergyOrthogonal = SSW_ORDER_ENERGY_ORTHOGONAL,
    Legacy = SSW_ORDER_LEGACY,
    Custom = SSW_ORDER_CUSTOM,
};

struct WriteConfig {                                   // algorithm.rs:99-112
    Insertion insertion = Insertion::Option2(0.1f);
    OrderingMethod ordering = OrderingMethod::Energy;
    ssw_precision precision = SSW_PRECISION_F64;
    ssw_config c() const { return {static_cast<int32_t>(ordering), insertion.method, insertion.alpha, precision}; }
};
struct ReadConfig {                                    // algorithm.rs:127-140
    Extraction extraction = Extraction::Option2(0.1f);
    OrderingMethod ordering = OrderingMethod::Energy;
    ssw_precision precision = SSW_PRECISION_F64;
    ssw_config c() const { return {static_cast<int32_t>(ordering), extraction.method, extraction.alpha, precision}; }
};

// An RGB f32 image [h][w][3].
struct ImageRgb32F {
    size_t width = 0, height = 0;
    std::vector<float> data;
    ImageRgb32F() = default;
    ImageRgb32F(size_t w, size_t h) : width(w), height(h), data(w * h * 3) {}
};

// An 8-bit RGB image [h][w][3] (what image files decode to).  Handed to the library as it is: `into_rgb32f()`
// (algorithm.rs:308, :476) runs on the device and a quarter of the bytes cross PCIe.
struct ImageRgb8 {
    size_t width = 0, height = 0;
    std::vector<uint8_t> data;
    ImageRgb8() = default;
    ImageRgb8(size_t w, size_t h) : width(w), height(h), data(w * h * 3) {}
};

// An 8-bit RGBA image [h][w][4]: a suspect whose alpha says where it has pixels of its own (tests/attack_crop.rs:56-70).
struct ImageRgba8 {
    size_t width = 0, height = 0;
    std::vector<uint8_t> data;
    ImageRgba8() = default;
    ImageRgba8(size_t w, size_t h) : width(w), height(h), data(w * h * 4) {}
};

// A 16-bit RGB image [h][w][3] (16-bit PNG / TIFF): `into_rgb32f()` = v / 65535 on the device, half the bytes cross PCIe.
struct ImageRgb16 {
    size_t width = 0, height = 0;
    std::vector<uint16_t> data;
    ImageRgb16() = default;
    ImageRgb16(size_t w, size_t h) : width(w), height(h), data(w * h * 3) {}
};

class MarkBuf {                                        // algorithm.rs:607-645
public:
    MarkBuf() = default;
    static MarkBuf generate_normal(size_t length) {    // :619-626 (non-deterministic by design)
        MarkBuf m;
        std::random_device rd;
        std::mt19937_64 gen(rd());
        std::normal_distribution<float> n(0.f, 1.f);
        m.data_.resize(length);
        for (auto& v : m.data_) v = n(gen);
        return m;
    }
    static MarkBuf from(const float* data, size_t n) { MarkBuf m; m.data_.assign(data, data + n); return m; }
    static MarkBuf from(const std::vector<float>& v) { return from(v.data(), v.size()); }
    const std::vector<float>& data() const { return data_; }
    void set_data(const float* data, size_t n) { data_.assign(data, data + n); }

private:
    std::vector<float> data_;
};

class Writer {                                         // algorithm.rs:285-433
public:
    Writer(Context& ctx, const ImageRgb32F& image, const WriteConfig& config = WriteConfig())
        : w_(image.width), h_(image.height) {
        if (image.data.size() != w_ * h_ * 3) throw Error(SSW_ERR_BAD_DIMS, "Writer::new");
        ssw_config c = config.c();
        check(ssw_writer_create(ctx.get(), image.data.data(), w_, h_, &c, &wr_), "Writer::new");
    }
    Writer(Context& ctx, const ImageRgb8& image, const WriteConfig& config = WriteConfig())
        : w_(image.width), h_(image.height) {
        if (image.data.size() != w_ * h_ * 3) throw Error(SSW_ERR_BAD_DIMS, "Writer::new");
        ssw_config c = config.c();
        check(ssw_writer_create_rgb8(ctx.get(), image.data.data(), w_, h_, &c, &wr_), "Writer::new");
    }
    Writer(Context& ctx, const ImageRgb16& image, const WriteConfig& config = WriteConfig())
        : w_(image.width), h_(image.height) {
        if (image.data.size() != w_ * h_ * 3) throw Error(SSW_ERR_BAD_DIMS, "Writer::new");
        ssw_config c = config.c();
        check(ssw_writer_create_rgb16(ctx.get(), image.data.data(), w_, h_, &c, &wr_), "Writer::new");
    }
    ~Writer() { ssw_writer_destroy(wr_); }
    Writer(const Writer&) = delete;
    Writer& operator=(const Writer&) = delete;

    std::vector<float> coefficient_image() const {     // :319-321
        std::vector<float> out(w_ * h_);
        check(ssw_writer_coefficients(wr_, out.data()), "Writer::coefficient_image");
        return out;
    }
    void embed(const std::vector<const MarkBuf*>& marks) {   // :348-352
        std::vector<const float*> p; std::vector<size_t> l;
        for (auto* m : marks) { p.push_back(m->data().data()); l.push_back(m->data().size()); }
        check(ssw_writer_embed(wr_, p.data(), l.data(), p.size()), "Writer::embed");
    }
    ImageRgb32F result() {                             // :361-379 (consumes the writer)
        ImageRgb32F out(w_, h_);
        check(ssw_writer_result(wr_, out.data.data()), "Writer::result");
        return out;
    }
    ImageRgb32F mark(const std::vector<const MarkBuf*>& marks) {   // :355-358
        embed(marks);
        return result();
    }
    // `writer.mark(marks).into_rgb8()` (examples/main.rs:271-278): quantised on the device, 3 bytes per pixel back
    ImageRgb8 mark_rgb8(const std::vector<const MarkBuf*>& marks) {
        embed(marks);
        ImageRgb8 out(w_, h_);
        check(ssw_writer_result_rgb8(wr_, out.data.data()), "Writer::mark");
        return out;
    }
    // Fingerprinting: for every mark what embed(&[&mark_i]) + result() would give on a clone of this writer as it stands
    // (:348-379, examples/main.rs:266-278 once per recipient).  Does not consume or change the writer; all marks one length.
    std::vector<ImageRgb32F> mark_copies(const std::vector<const MarkBuf*>& marks) {
        return copies<ImageRgb32F>(marks, ssw_writer_mark_copies);
    }
    std::vector<ImageRgb8> mark_copies_rgb8(const std::vector<const MarkBuf*>& marks) {
        return copies<ImageRgb8>(marks, ssw_writer_mark_copies_rgb8);
    }

private:
    template <class Img, class Fn>
    std::vector<Img> copies(const std::vector<const MarkBuf*>& marks, Fn fn) {
        const size_t n = marks.size(), k = n ? marks[0]->data().size() : 0;
        std::vector<float> m(n * k);
        for (size_t i = 0; i < n; ++i) {
            if (marks[i]->data().size() != k) throw Error(SSW_ERR_LENGTH_MISMATCH, "Writer::mark_copies");
            std::copy(marks[i]->data().begin(), marks[i]->data().end(), m.begin() + i * k);
        }
        std::vector<typename decltype(Img::data)::value_type> all(n * w_ * h_ * 3);
        check(fn(wr_, m.data(), n, k, all.data()), "Writer::mark_copies");
        std::vector<Img> out;
        for (size_t i = 0; i < n; ++i) {
            out.emplace_back(w_, h_);
            std::copy(all.begin() + i * w_ * h_ * 3, all.begin() + (i + 1) * w_ * h_ * 3, out.back().data.begin());
        }
        return out;
    }
    size_t w_, h_;
    ssw_writer* wr_ = nullptr;
};

class ReaderDerived;

// What Reader::trace returns, per suspect s: extracted[s] (k values), sims[s] (one per mark; the GEMM matrix, 1e-4 relative),
// best[s] (index of the strongest mark, TraceResult::none without one), best_sim[s] (Tester::similarity of that mark, exact;
// NaN without one), n_exceed[s] (marks above the threshold: two and more = colluders -- for an averaged forgery; see the
// strength report: wm::collude, wm::quality).
struct TraceResult {
    static constexpr uint32_t none = 0xFFFFFFFFu;
    std::vector<std::vector<float>> extracted, sims;
    std::vector<uint32_t> best, n_exceed;
    std::vector<float> best_sim;
};

// Where a suspect lies in the original's frame (ssw_placement): the rectangle at (x, y) of size w x h; w = h = 0: the suspect's
// own size.  Placement::whole_frame(original) is the placement of a scaled copy.
struct Placement {
    size_t x = 0, y = 0, w = 0, h = 0;
    template <class Image> static Placement whole_frame(const Image& original) { return Placement{0, 0, original.width, original.height}; }
};
// A suspect of Reader::trace with placements: an RGB or RGBA image of any size, not owned
struct Suspect {
    const uint8_t* data;
    size_t width, height, channels;
    Suspect(const ImageRgb8& im) : data(im.data.data()), width(im.width), height(im.height), channels(3) { if (im.data.size() != width * height * 3) throw Error(SSW_ERR_BAD_DIMS, "Suspect"); }
    Suspect(const ImageRgba8& im) : data(im.data.data()), width(im.width), height(im.height), channels(4) { if (im.data.size() != width * height * 4) throw Error(SSW_ERR_BAD_DIMS, "Suspect"); }
};

// Where a cut-out lies: the complete placement (ready for Reader::trace), the luma SAD there and the same per pixel
struct Located {
    Placement placement;
    uint64_t sad = 0;
    double mean_abs_diff = 0.0;
};
// ssw_locate_rgb8 on host images: finds each suspect in `original` by translation.  sizes[i]: the size suspect i had in the
// original's frame ({0, 0}: its own; x, y of the entry are not read); an empty `sizes`: every suspect at its own size.
inline std::vector<Located> locate(Context& ctx, const ImageRgb8& original, const std::vector<Suspect>& suspects,
                                   const std::vector<Placement>& sizes = {}) {
    const size_t n = suspects.size();
    if ((!sizes.empty() && sizes.size() != n) || original.data.size() != original.width * original.height * 3) throw Error(SSW_ERR_BAD_DIMS, "locate");
    std::vector<void*> dev(n + 1, nullptr);
    struct Free {
        ssw_ctx* c; std::vector<void*>& d;
        ~Free() { for (void* p : d) if (p) ssw_dev_free(c, p); }
    } guard{ctx.get(), dev};
    auto put = [&](const void* src, size_t bytes, void** out) {
        check(ssw_dev_alloc(ctx.get(), bytes, out), "locate");
        check(ssw_copy_to_dev(ctx.get(), *out, src, bytes), "locate");
    };
    put(original.data.data(), original.data.size(), &dev[n]);
    std::vector<ssw_placement> pl(n);
    for (size_t i = 0; i < n; ++i) {
        put(suspects[i].data, suspects[i].width * suspects[i].height * suspects[i].channels, &dev[i]);
        const Placement s = sizes.empty() ? Placement() : sizes[i];
        pl[i] = ssw_placement{(uint32_t)suspects[i].width, (uint32_t)suspects[i].height, (uint32_t)suspects[i].channels, 0u, 0u, (uint32_t)s.w, (uint32_t)s.h};
    }
    std::vector<uint64_t> sad(n);
    check(ssw_locate_rgb8(ctx.get(), static_cast<const uint8_t*>(dev[n]), original.width, original.height, dev.data(), pl.data(), n, sad.data()), "locate");
    std::vector<Located> out(n);
    for (size_t i = 0; i < n; ++i) {
        const size_t pw = pl[i].pw ? pl[i].pw : pl[i].w, ph = pl[i].ph ? pl[i].ph : pl[i].h;
        out[i] = Located{Placement{pl[i].x, pl[i].y, pw, ph}, sad[i], (double)sad[i] / ((double)pw * (double)ph)};
    }
    return out;
}

// The widths a cut-out may have had in the original (ssw_scale_range): its scale is not known
struct ScaleRange {
    size_t wmin = 0, wmax = 0;
};
// ssw_locate_scaled_rgb8 on host images: finds each suspect in `original` by translation AND scale (aspect ratio kept, the
// smaller side at least 32); Located::placement carries the size that was found.
inline std::vector<Located> locate_scaled(Context& ctx, const ImageRgb8& original, const std::vector<Suspect>& suspects,
                                          const std::vector<ScaleRange>& ranges) {
    const size_t n = suspects.size();
    if (ranges.size() != n || original.data.size() != original.width * original.height * 3) throw Error(SSW_ERR_BAD_DIMS, "locate_scaled");
    std::vector<void*> dev(n + 1, nullptr);
    struct Free {
        ssw_ctx* c; std::vector<void*>& d;
        ~Free() { for (void* p : d) if (p) ssw_dev_free(c, p); }
    } guard{ctx.get(), dev};
    auto put = [&](const void* src, size_t bytes, void** out) {
        check(ssw_dev_alloc(ctx.get(), bytes, out), "locate_scaled");
        check(ssw_copy_to_dev(ctx.get(), *out, src, bytes), "locate_scaled");
    };
    put(original.data.data(), original.data.size(), &dev[n]);
    std::vector<ssw_placement> pl(n);
    std::vector<ssw_scale_range> rg(n);
    for (size_t i = 0; i < n; ++i) {
        put(suspects[i].data, suspects[i].width * suspects[i].height * suspects[i].channels, &dev[i]);
        pl[i] = ssw_placement{(uint32_t)suspects[i].width, (uint32_t)suspects[i].height, (uint32_t)suspects[i].channels, 0u, 0u, 0u, 0u};
        rg[i] = ssw_scale_range{(uint32_t)ranges[i].wmin, (uint32_t)ranges[i].wmax};
    }
    std::vector<uint64_t> sad(n);
    check(ssw_locate_scaled_rgb8(ctx.get(), static_cast<const uint8_t*>(dev[n]), original.width, original.height, dev.data(), pl.data(), rg.data(), n, sad.data()), "locate_scaled");
    std::vector<Located> out(n);
    for (size_t i = 0; i < n; ++i)
        out[i] = Located{Placement{pl[i].x, pl[i].y, pl[i].pw, pl[i].ph}, sad[i], (double)sad[i] / ((double)pl[i].pw * (double)pl[i].ph)};
    return out;
}

// ssw_signature_host_rgb8 on host images of any sizes: 1024 bytes per image, in the order of `images`.
inline std::vector<std::array<uint8_t, 1024>> signature(Context& ctx, const std::vector<Suspect>& images) {
    const size_t n = images.size();
    std::vector<const uint8_t*> ptrs(n);
    std::vector<ssw_image_shape> shapes(n);
    for (size_t i = 0; i < n; ++i) {
        ptrs[i] = images[i].data;
        shapes[i] = ssw_image_shape{(uint32_t)images[i].width, (uint32_t)images[i].height, (uint32_t)images[i].channels};
    }
    std::vector<std::array<uint8_t, 1024>> out(n);
    check(ssw_signature_host_rgb8(ctx.get(), ptrs.data(), shapes.data(), n, n ? out[0].data() : nullptr), "signature");
    return out;
}

// How far a copy is from its original (ssw_quality_rgb8): squared error per channel and of the luma, changed bytes, the largest
// byte difference; PSNR is the caller's arithmetic on them.
struct Quality {
    uint64_t sse[3] = {0, 0, 0}, sse_luma = 0, changed = 0, max_abs = 0, pixels = 0;
    double psnr() const {
        const double e = (double)sse[0] + (double)sse[1] + (double)sse[2];
        return e == 0.0 ? std::numeric_limits<double>::infinity() : 10.0 * std::log10(255.0 * 255.0 * 3.0 * (double)pixels / e);
    }
    double psnr_luma() const {
        return sse_luma == 0 ? std::numeric_limits<double>::infinity() : 10.0 * std::log10(255.0 * 255.0 * (double)pixels / (double)sse_luma);
    }
    double changed_fraction() const { return pixels ? (double)changed / (3.0 * (double)pixels) : 0.0; }
};
// One forgery of wm::collude: a method and 1 .. 16 indices into the copies (repeats allowed)
struct Coalition {
    ssw_collude_method method = SSW_COLLUDE_AVERAGE;
    std::vector<uint32_t> members;
};
namespace detail {
// n host frames of one size, one after the other on the device; freed with the object
struct DeviceFrames {
    ssw_ctx* c;
    uint8_t* p = nullptr;
    DeviceFrames(ssw_ctx* ctx, size_t bytes, const char* where) : c(ctx) { check(ssw_dev_alloc(c, bytes ? bytes : 16, reinterpret_cast<void**>(&p)), where); }
    ~DeviceFrames() { if (p) ssw_dev_free(c, p); }
    DeviceFrames(const DeviceFrames&) = delete;
    DeviceFrames& operator=(const DeviceFrames&) = delete;
    void put(const std::vector<const ImageRgb8*>& images, size_t w, size_t h, const char* where) {
        for (size_t i = 0; i < images.size(); ++i) {
            if (images[i]->width != w || images[i]->height != h || images[i]->data.size() != w * h * 3) throw Error(SSW_ERR_BAD_DIMS, where);
            check(ssw_copy_to_dev(c, p + i * w * h * 3, images[i]->data.data(), w * h * 3), where);
        }
    }
};
// ssw_quality_rgb8, ssw_ssim_rgb8: every copy against the one original through run(dev_base, dev_copies, n, dev_stats); the
// S words a copy's statistics take come back one copy after the other.
template <size_t S, class Run>
std::vector<uint64_t> against_original(Context& ctx, const ImageRgb8& original, const std::vector<const ImageRgb8*>& copies, const char* where, Run run) {
    const size_t n = copies.size(), w = original.width, h = original.height, fb = w * h * 3;
    DeviceFrames base(ctx.get(), fb, where), dev(ctx.get(), n * fb, where), st(ctx.get(), n * S * sizeof(uint64_t), where);
    base.put({&original}, w, h, where);
    dev.put(copies, w, h, where);
    check(run(base.p, dev.p, n, reinterpret_cast<uint64_t*>(st.p)), where);
    std::vector<uint64_t> raw(n * S);
    check(ssw_copy_to_host(ctx.get(), raw.data(), st.p, raw.size() * sizeof(uint64_t)), where);
    return raw;
}
// ssw_collude_rgb8, ssw_jpeg_rgb8, ssw_filter_rgb8: the frames go up, call(ctx, dev_frames, n, w, h, jobs, m, dev_out) writes one
// frame per job, and the m frames come down.
template <class Job, class Call>
std::vector<ImageRgb8> frames_through_jobs(Context& ctx, const std::vector<const ImageRgb8*>& frames, const std::vector<Job>& jobs, const char* where, Call call) {
    if (frames.empty()) throw Error(SSW_ERR_BAD_ARG, where);
    const size_t n = frames.size(), m = jobs.size(), w = frames[0]->width, h = frames[0]->height, fb = w * h * 3;
    DeviceFrames dev(ctx.get(), n * fb, where), made(ctx.get(), m * fb, where);
    dev.put(frames, w, h, where);
    check(call(ctx.get(), dev.p, n, w, h, jobs.data(), m, made.p), where);
    std::vector<ImageRgb8> out(m, ImageRgb8(w, h));
    for (size_t i = 0; i < m; ++i) check(ssw_copy_to_host(ctx.get(), out[i].data.data(), made.p + i * fb, fb), where);
    return out;
}
}  // namespace detail
// ssw_quality_rgb8 on host images: every copy against the one original.
inline std::vector<Quality> quality(Context& ctx, const ImageRgb8& original, const std::vector<const ImageRgb8*>& copies) {
    const size_t w = original.width, h = original.height;
    const auto run = [&](const uint8_t* base, const uint8_t* dev, size_t n, uint64_t* st) { return ssw_quality_rgb8(ctx.get(), base, 1, dev, n, w, h, st); };
    const std::vector<uint64_t> raw = detail::against_original<6>(ctx, original, copies, "quality", run);
    std::vector<Quality> out(copies.size());
    for (size_t i = 0; i < out.size(); ++i) {
        const uint64_t* r = &raw[i * 6];
        out[i].sse[0] = r[0]; out[i].sse[1] = r[1]; out[i].sse[2] = r[2];
        out[i].sse_luma = r[3]; out[i].changed = r[4]; out[i].max_abs = r[5]; out[i].pixels = w * h;
    }
    return out;
}
// The structural similarity of a copy and its original (ssw_ssim_rgb8; include/ssw.h states the definition): the sum of the
// windows' fixed-point values (SSW_SSIM_ONE = identical) and the worst window with the pixel of its upper left corner; the mean
// is the caller's arithmetic on them.
struct Ssim {
    int64_t sum = 0;
    int32_t worst = 0;
    uint32_t worst_x = 0, worst_y = 0;
    uint64_t windows = 0;
    double mean() const { return windows ? (double)sum / ((double)SSW_SSIM_ONE * (double)windows) : 0.0; }
    double worst_value() const { return (double)worst / (double)SSW_SSIM_ONE; }
};
// ssw_ssim_rgb8 on host images: every copy against the one original.  No side below SSW_SSIM_MIN_SIDE.
inline std::vector<Ssim> ssim(Context& ctx, const ImageRgb8& original, const std::vector<const ImageRgb8*>& copies) {
    const size_t w = original.width, h = original.height;
    if (w < SSW_SSIM_MIN_SIDE || h < SSW_SSIM_MIN_SIDE) throw Error(SSW_ERR_BAD_ARG, "ssim");
    const size_t nx = w / 4 - 1, ny = h / 4 - 1;
    const auto run = [&](const uint8_t* base, const uint8_t* dev, size_t n, uint64_t* st) { return ssw_ssim_rgb8(ctx.get(), base, 1, dev, n, w, h, st, nullptr); };
    const std::vector<uint64_t> raw = detail::against_original<SSW_SSIM_STATS>(ctx, original, copies, "ssim", run);
    std::vector<Ssim> out(copies.size());
    for (size_t i = 0; i < out.size(); ++i) {
        const uint64_t key = raw[i * SSW_SSIM_STATS + 1], index = key & 0xFFFFFFFFull;
        out[i].sum = (int64_t)raw[i * SSW_SSIM_STATS];
        out[i].worst = (int32_t)((int64_t)(key >> 32) - SSW_SSIM_ONE);
        out[i].worst_x = (uint32_t)(index % nx * 4); out[i].worst_y = (uint32_t)(index / nx * 4);
        out[i].windows = nx * ny;
    }
    return out;
}
// ssw_collude_rgb8 on host images of one size: one forged frame per coalition, in order.
inline std::vector<ImageRgb8> collude(Context& ctx, const std::vector<const ImageRgb8*>& copies, const std::vector<Coalition>& coalitions) {
    std::vector<ssw_coalition> co(coalitions.size());
    for (size_t i = 0; i < co.size(); ++i) {
        if (coalitions[i].members.empty() || coalitions[i].members.size() > 16) throw Error(SSW_ERR_BAD_ARG, "collude");
        co[i] = ssw_coalition{(uint32_t)coalitions[i].method, (uint32_t)coalitions[i].members.size(), {}};
        std::copy(coalitions[i].members.begin(), coalitions[i].members.end(), co[i].member);
    }
    return detail::frames_through_jobs(ctx, copies, co, "collude", ssw_collude_rgb8);
}

// One result of wm::jpeg: a frame (an index into the images) and a JPEG quality 1 .. 100
struct JpegJob {
    uint32_t frame = 0;
    uint32_t quality = 75;
};
// ssw_jpeg_rgb8 on host images of one size: per job that frame as it comes back from a baseline JPEG of that quality -- what
// libjpeg-turbo's defaults (4:2:0, islow DCT, fancy upsampling) give, byte for byte; include/ssw.h states the steps.
inline std::vector<ImageRgb8> jpeg(Context& ctx, const std::vector<const ImageRgb8*>& frames, const std::vector<JpegJob>& jobs) {
    std::vector<ssw_jpeg_job> jb(jobs.size());
    for (size_t i = 0; i < jb.size(); ++i) jb[i] = ssw_jpeg_job{jobs[i].frame, jobs[i].quality};
    return detail::frames_through_jobs(ctx, frames, jb, "jpeg", ssw_jpeg_rgb8);
}

// One result of wm::filter: a frame (an index into the images) and one of the three filters of ssw_filter_rgb8
struct FilterJob {
    uint32_t frame = 0;
    uint32_t kind = SSW_FILTER_MEDIAN3;
    float radius = 0.0f;                  // blur, unsharp: the Gaussian's sigma, 0 < radius <= 8
    uint32_t percent = 0, threshold = 0;  // unsharp: 1 .. 1000 and 0 .. 255
    static FilterJob blur(uint32_t frame, float radius) { return FilterJob{frame, SSW_FILTER_BLUR, radius, 0, 0}; }
    static FilterJob unsharp(uint32_t frame, float radius = 2.0f, uint32_t percent = 150, uint32_t threshold = 3) {
        return FilterJob{frame, SSW_FILTER_UNSHARP, radius, percent, threshold};
    }
    static FilterJob median(uint32_t frame) { return FilterJob{frame, SSW_FILTER_MEDIAN3, 0.0f, 0, 0}; }
};
// ssw_filter_rgb8 on host images of one size: per job that frame after a Gaussian blur, an unsharp mask or a 3 x 3 median -- what
// Pillow's filters of those names give, byte for byte; include/ssw.h states the definitions.
inline std::vector<ImageRgb8> filter(Context& ctx, const std::vector<const ImageRgb8*>& frames, const std::vector<FilterJob>& jobs) {
    std::vector<ssw_filter_job> jb(jobs.size());
    for (size_t i = 0; i < jb.size(); ++i) jb[i] = ssw_filter_job{jobs[i].frame, jobs[i].kind, jobs[i].radius, jobs[i].percent, jobs[i].threshold};
    return detail::frames_through_jobs(ctx, frames, jb, "filter", ssw_filter_rgb8);
}

// The filters of Pillow's Image.resize that ssw_resample_rgb8 offers
enum class ResampleFilter : uint32_t { Box = SSW_RESAMPLE_BOX, Bilinear = SSW_RESAMPLE_BILINEAR, Bicubic = SSW_RESAMPLE_BICUBIC, Lanczos = SSW_RESAMPLE_LANCZOS };
// ssw_resample_rgb8 on host images of one size: every image as PIL.Image.resize((nw, nh), filter) makes it, byte for byte;
// include/ssw.h states the definition.
inline std::vector<ImageRgb8> resample(Context& ctx, const std::vector<const ImageRgb8*>& frames, size_t nw, size_t nh,
                                       ResampleFilter filter = ResampleFilter::Bicubic) {
    if (frames.empty()) throw Error(SSW_ERR_BAD_ARG, "resample");
    const size_t n = frames.size(), w = frames[0]->width, h = frames[0]->height, ob = nw * nh * 3;
    detail::DeviceFrames dev(ctx.get(), n * w * h * 3, "resample"), made(ctx.get(), n * ob, "resample");
    dev.put(frames, w, h, "resample");
    check(ssw_resample_rgb8(ctx.get(), dev.p, n, w, h, nw, nh, (int)filter, made.p), "resample");
    std::vector<ImageRgb8> out(n, ImageRgb8(nw, nh));
    for (size_t i = 0; i < n; ++i) check(ssw_copy_to_host(ctx.get(), out[i].data.data(), made.p + i * ob, ob), "resample");
    return out;
}
// One result of wm::scale_attack: a frame (an index into the images), the thumbnail's size and the filter that makes it
struct Scale {
    uint32_t frame = 0;
    uint32_t nw = 1, nh = 1;
    ResampleFilter filter = ResampleFilter::Bicubic;
    // the thumbnail of a w x h frame at `factor`: sides rounded half up, at least 1
    static Scale by(uint32_t frame, size_t w, size_t h, double factor, ResampleFilter filter = ResampleFilter::Bicubic) {
        const auto side = [&](size_t v) { const long s = (long)((double)v * factor + 0.5); return (uint32_t)(s < 1 ? 1 : s); };
        return Scale{frame, side(w), side(h), filter};
    }
};
// ssw_scale_attack_rgb8 on host images of one size: per job that frame scaled as Pillow's Image.resize does it and brought back
// to its size as a trace brings back a suspect of another size; include/ssw.h states both steps.
inline std::vector<ImageRgb8> scale_attack(Context& ctx, const std::vector<const ImageRgb8*>& frames, const std::vector<Scale>& jobs) {
    std::vector<ssw_scale_job> jb(jobs.size());
    for (size_t i = 0; i < jb.size(); ++i) jb[i] = ssw_scale_job{jobs[i].frame, jobs[i].nw, jobs[i].nh, (uint32_t)jobs[i].filter};
    return detail::frames_through_jobs(ctx, frames, jb, "scale_attack", ssw_scale_attack_rgb8);
}

// The filters of Pillow's Image.rotate / Image.transform that ssw_affine_rgb8 offers
enum class AffineFilter : uint32_t { Bilinear = SSW_AFFINE_BILINEAR, Bicubic = SSW_AFFINE_BICUBIC };
using Matrix = std::array<double, 6>;
// PIL.Image.rotate(angle)'s matrix for a w x h frame (ssw_rotation_matrix)
inline Matrix rotation_matrix(double angle, size_t w, size_t h) {
    Matrix m{};
    check(ssw_rotation_matrix(angle, w, h, m.data()), "rotation_matrix");
    return m;
}
// ssw_affine_rgb8 on host images of one size: every image as PIL.Image.transform((ow, oh), AFFINE, m, filter, fillcolor=fill)
// makes it, byte for byte; include/ssw.h states the definition.
inline std::vector<ImageRgb8> affine(Context& ctx, const std::vector<const ImageRgb8*>& frames, size_t ow, size_t oh, const Matrix& m,
                                     AffineFilter filter = AffineFilter::Bicubic, const std::array<uint8_t, 3>& fill = {0, 0, 0}) {
    if (frames.empty()) throw Error(SSW_ERR_BAD_ARG, "affine");
    const size_t n = frames.size(), w = frames[0]->width, h = frames[0]->height, ob = ow * oh * 3;
    detail::DeviceFrames dev(ctx.get(), n * w * h * 3, "affine"), made(ctx.get(), n * ob, "affine");
    dev.put(frames, w, h, "affine");
    check(ssw_affine_rgb8(ctx.get(), dev.p, n, w, h, ow, oh, m.data(), (int)filter, fill.data(), made.p), "affine");
    std::vector<ImageRgb8> out(n, ImageRgb8(ow, oh));
    for (size_t i = 0; i < n; ++i) check(ssw_copy_to_host(ctx.get(), out[i].data.data(), made.p + i * ob, ob), "affine");
    return out;
}
// every image as PIL.Image.rotate(angle, filter, fillcolor=fill) makes it
inline std::vector<ImageRgb8> rotate(Context& ctx, const std::vector<const ImageRgb8*>& frames, double angle, AffineFilter filter = AffineFilter::Bicubic,
                                     const std::array<uint8_t, 3>& fill = {0, 0, 0}) {
    if (frames.empty()) throw Error(SSW_ERR_BAD_ARG, "rotate");
    return affine(ctx, frames, frames[0]->width, frames[0]->height, rotation_matrix(angle, frames[0]->width, frames[0]->height), filter, fill);
}
// One result of wm::rotate_attack / wm::unrotate: a frame (an index into the images), the angle it is (or was) turned by, and
// the filter and fill of the attack
struct Rotate {
    uint32_t frame = 0;
    double angle = 0.0;
    AffineFilter filter = AffineFilter::Bicubic;
    std::array<uint8_t, 3> fill{{0, 0, 0}};
    ssw_rotate_job job(size_t w, size_t h) const {
        ssw_rotate_job j{};
        j.frame = frame; j.filter = (uint32_t)filter;
        for (int c = 0; c < 3; ++c) j.fill[c] = fill[c];
        const Matrix f = rotation_matrix(angle, w, h), b = rotation_matrix(-angle, w, h);
        for (int i = 0; i < 6; ++i) { j.forward[i] = f[i]; j.back[i] = b[i]; }
        return j;
    }
};
// ssw_rotate_attack_rgb8 on host images of one size: per job that frame turned as Pillow's Image.rotate does it, then turned
// back by the known angle and completed with `original` where the turns lost pixels; include/ssw.h states both steps.
inline std::vector<ImageRgb8> rotate_attack(Context& ctx, const ImageRgb8& original, const std::vector<const ImageRgb8*>& frames,
                                            const std::vector<Rotate>& jobs) {
    const size_t w = original.width, h = original.height;
    detail::DeviceFrames base(ctx.get(), w * h * 3, "rotate_attack");
    base.put({&original}, w, h, "rotate_attack");
    std::vector<ssw_rotate_job> jb(jobs.size());
    for (size_t i = 0; i < jb.size(); ++i) jb[i] = jobs[i].job(w, h);
    const auto call = [&](ssw_ctx* c, const uint8_t* dev, size_t n, size_t fw, size_t fh, const ssw_rotate_job* j, size_t m, uint8_t* out) {
        return ssw_rotate_attack_rgb8(c, base.p, dev, n, fw, fh, j, m, out);
    };
    return detail::frames_through_jobs(ctx, frames, jb, "rotate_attack", call);
}
// ssw_unrotate_rgb8 on host images of the original's size: suspect i turned back by angles[i] and completed with `original`:
// what tracing a copy that was turned by a known angle extracts from.
inline std::vector<ImageRgb8> unrotate(Context& ctx, const ImageRgb8& original, const std::vector<const ImageRgb8*>& suspects,
                                       const std::vector<double>& angles) {
    if (angles.size() != suspects.size()) throw Error(SSW_ERR_BAD_ARG, "unrotate");
    const size_t w = original.width, h = original.height;
    detail::DeviceFrames base(ctx.get(), w * h * 3, "unrotate");
    base.put({&original}, w, h, "unrotate");
    std::vector<ssw_rotate_job> jb(angles.size());
    for (size_t i = 0; i < jb.size(); ++i) jb[i] = Rotate{(uint32_t)i, angles[i]}.job(w, h);
    const auto call = [&](ssw_ctx* c, const uint8_t* dev, size_t n, size_t fw, size_t fh, const ssw_rotate_job* j, size_t, uint8_t* out) {
        return ssw_unrotate_rgb8(c, base.p, dev, n, fw, fh, j, out);
    };
    return detail::frames_through_jobs(ctx, suspects, jb, "unrotate", call);
}

// The originals someone owns, as signatures: which of them is a suspect a copy of?  The stage in front of locate / Reader::trace
// (ssw_signature_match; include/ssw.h states the definition and what it cannot find: cut-outs, mirrored and turned copies).
// The signatures stay on the device between match calls and go up again only after an add.
class Catalogue {
public:
    struct Match {
        static constexpr uint32_t none = 0xFFFFFFFFu;
        uint32_t index = none, distance = none;        // position among the entries added; both `none` beyond the catalogue's size
    };
    explicit Catalogue(Context& ctx) : ctx_(ctx) {}
    ~Catalogue() { if (dev_) ssw_dev_free(ctx_.get(), dev_); }
    Catalogue(const Catalogue&) = delete;
    Catalogue& operator=(const Catalogue&) = delete;
    size_t size() const { return names_.size(); }
    const std::string& name(size_t i) const { return names_[i]; }
    void add(const std::string& name, const Suspect& image) {
        const auto sig = signature(ctx_, {image});
        names_.push_back(name);
        sigs_.insert(sigs_.end(), sig[0].begin(), sig[0].end());
    }
    // per suspect the `top` (1 .. 8) nearest entries, nearest first, ties to the lower index
    std::vector<std::vector<Match>> match(const std::vector<Suspect>& suspects, size_t top = 1) {
        const size_t nq = suspects.size();
        std::vector<std::vector<Match>> out(nq, std::vector<Match>(top));
        if (nq == 0) return out;
        const auto q = signature(ctx_, suspects);
        if (dev_n_ != size()) {
            if (dev_) check(ssw_dev_free(ctx_.get(), dev_), "Catalogue::match");
            dev_ = nullptr;
            if (size()) {
                check(ssw_dev_alloc(ctx_.get(), sigs_.size(), &dev_), "Catalogue::match");
                check(ssw_copy_to_dev(ctx_.get(), dev_, sigs_.data(), sigs_.size()), "Catalogue::match");
            }
            dev_n_ = size();
        }
        void* dq = nullptr;
        void* res = nullptr;
        struct Free {
            ssw_ctx* c; void*& a; void*& b;
            ~Free() { if (a) ssw_dev_free(c, a); if (b) ssw_dev_free(c, b); }
        } guard{ctx_.get(), dq, res};
        check(ssw_dev_alloc(ctx_.get(), nq * 1024, &dq), "Catalogue::match");
        check(ssw_copy_to_dev(ctx_.get(), dq, q[0].data(), nq * 1024), "Catalogue::match");
        check(ssw_dev_alloc(ctx_.get(), 2 * nq * top * sizeof(uint32_t), &res), "Catalogue::match");
        uint32_t* idx = static_cast<uint32_t*>(res);
        check(ssw_signature_match(ctx_.get(), static_cast<const uint8_t*>(dq), nq, static_cast<const uint8_t*>(dev_), size(), top, idx,
                                  idx + nq * top, nullptr), "Catalogue::match");
        std::vector<uint32_t> host(2 * nq * top);
        check(ssw_copy_to_host(ctx_.get(), host.data(), res, host.size() * sizeof(uint32_t)), "Catalogue::match");
        for (size_t s = 0; s < nq; ++s)
            for (size_t t = 0; t < top; ++t) out[s][t] = Match{host[s * top + t], host[(nq + s) * top + t]};
        return out;
    }

private:
    Context& ctx_;
    std::vector<std::string> names_;
    std::vector<uint8_t> sigs_;
    void* dev_ = nullptr;
    size_t dev_n_ = 0;
};

class Reader {                                         // algorithm.rs:441-594
public:
    static Reader base(Context& ctx, const ImageRgb32F& image, const ReadConfig& config = ReadConfig()) {   // :462-464
        return Reader(ctx, image, true, config);
    }
    static Reader base(Context& ctx, const ImageRgb8& image, const ReadConfig& config = ReadConfig()) {
        return Reader(ctx, image, true, config);
    }
    static Reader base(Context& ctx, const ImageRgb16& image, const ReadConfig& config = ReadConfig()) {
        return Reader(ctx, image, true, config);
    }
    ~Reader() { ssw_reader_destroy(rd_); }
    Reader(Reader&& o) noexcept : w_(o.w_), h_(o.h_), rd_(o.rd_) { o.rd_ = nullptr; }
    Reader(const Reader&) = delete;
    Reader& operator=(const Reader&) = delete;

    std::vector<float> coefficients() const {          // :502-504
        std::vector<float> out(w_ * h_);
        check(ssw_reader_coefficients(rd_, out.data()), "Reader::coefficients");
        return out;
    }
    std::vector<uint64_t> indices(size_t k) const {    // :506-508 (first k entries)
        std::vector<uint64_t> out(k);
        check(ssw_reader_indices(rd_, k, out.data()), "Reader::indices");
        return out;
    }
    void extract(const ReaderDerived& derived, std::vector<float>& extracted) const;   // :529-539
    // Whose copy is each suspect?  extract() against every suspect and Tester::similarity against every stored mark
    // (:529-539, :696-714; the `test` loop of examples/main.rs:369-415) as one call on this base reader's plane and index
    // list (a derived reader: SSW_ERR_NOT_BASE).  All marks one length; suspects of the reader's size.
    TraceResult trace(const std::vector<const ImageRgb8*>& suspects, const std::vector<const MarkBuf*>& marks, float threshold = 6.0f) const {
        const size_t n = suspects.size(), nm = marks.size(), k = nm ? marks[0]->data().size() : 0;
        std::vector<const uint8_t*> sp(n);
        for (size_t i = 0; i < n; ++i) {
            if (suspects[i]->width != w_ || suspects[i]->height != h_ || suspects[i]->data.size() != w_ * h_ * 3) throw Error(SSW_ERR_BAD_DIMS, "Reader::trace");
            sp[i] = suspects[i]->data.data();
        }
        std::vector<float> m(nm * k), ext(n * k), sims(n * nm);
        for (size_t j = 0; j < nm; ++j) {
            if (marks[j]->data().size() != k) throw Error(SSW_ERR_LENGTH_MISMATCH, "Reader::trace");
            std::copy(marks[j]->data().begin(), marks[j]->data().end(), m.begin() + j * k);
        }
        TraceResult r;
        r.best.assign(n, TraceResult::none); r.n_exceed.assign(n, 0u); r.best_sim.assign(n, std::nanf(""));
        check(ssw_reader_trace_host_rgb8(rd_, sp.data(), n, k, nm ? m.data() : nullptr, nm, threshold, ext.data(), nm ? sims.data() : nullptr,
                                         nm ? r.best.data() : nullptr, nm ? r.best_sim.data() : nullptr, nm ? r.n_exceed.data() : nullptr),
              "Reader::trace");
        for (size_t i = 0; i < n; ++i) {
            r.extracted.emplace_back(ext.begin() + i * k, ext.begin() + (i + 1) * k);
            r.sims.emplace_back(sims.begin() + i * nm, sims.begin() + (i + 1) * nm);
        }
        return r;
    }
    // The same for attacked copies: each suspect (RGB or RGBA, any size) is first restored on the device -- resized into the
    // rectangle its placement names (tests/attack_resize.rs:31-36) and blended over the original (tests/attack_crop.rs:56-70);
    // ssw_restore_rgb8 in ssw.h has the recipe.  `original`: the pixels this base reader was made from (it keeps the plane
    // and the list, not the image).
    TraceResult trace(const ImageRgb8& original, const std::vector<Suspect>& suspects, const std::vector<Placement>& placements,
                      const std::vector<const MarkBuf*>& marks, float threshold = 6.0f) const {
        const size_t n = suspects.size(), nm = marks.size(), k = nm ? marks[0]->data().size() : 0;
        if (placements.size() != n || original.width != w_ || original.height != h_ || original.data.size() != w_ * h_ * 3)
            throw Error(SSW_ERR_BAD_DIMS, "Reader::trace");
        std::vector<const uint8_t*> sp(n);
        std::vector<ssw_placement> pl(n);
        for (size_t i = 0; i < n; ++i) {
            sp[i] = suspects[i].data;
            pl[i] = ssw_placement{(uint32_t)suspects[i].width, (uint32_t)suspects[i].height, (uint32_t)suspects[i].channels,
                                  (uint32_t)placements[i].x, (uint32_t)placements[i].y, (uint32_t)placements[i].w, (uint32_t)placements[i].h};
        }
        std::vector<float> m(nm * k), ext(n * k), sims(n * nm);
        for (size_t j = 0; j < nm; ++j) {
            if (marks[j]->data().size() != k) throw Error(SSW_ERR_LENGTH_MISMATCH, "Reader::trace");
            std::copy(marks[j]->data().begin(), marks[j]->data().end(), m.begin() + j * k);
        }
        TraceResult r;
        r.best.assign(n, TraceResult::none); r.n_exceed.assign(n, 0u); r.best_sim.assign(n, std::nanf(""));
        check(ssw_reader_trace_restored_host_rgb8(rd_, original.data.data(), sp.data(), pl.data(), n, k, nm ? m.data() : nullptr, nm, threshold,
                                                  ext.data(), nm ? sims.data() : nullptr, nm ? r.best.data() : nullptr,
                                                  nm ? r.best_sim.data() : nullptr, nm ? r.n_exceed.data() : nullptr),
              "Reader::trace");
        for (size_t i = 0; i < n; ++i) {
            r.extracted.emplace_back(ext.begin() + i * k, ext.begin() + (i + 1) * k);
            r.sims.emplace_back(sims.begin() + i * nm, sims.begin() + (i + 1) * nm);
        }
        return r;
    }

private:
    friend class ReaderDerived;
    Reader(Context& ctx, const ImageRgb32F& image, bool is_base, const ReadConfig& config)
        : w_(image.width), h_(image.height) {
        if (image.data.size() != w_ * h_ * 3) throw Error(SSW_ERR_BAD_DIMS, "Reader::new_impl");
        ssw_config c = config.c();
        check(ssw_reader_create(ctx.get(), image.data.data(), w_, h_, is_base ? 1 : 0, &c, &rd_), "Reader::new_impl");
    }
    Reader(Context& ctx, const ImageRgb8& image, bool is_base, const ReadConfig& config)
        : w_(image.width), h_(image.height) {
        if (image.data.size() != w_ * h_ * 3) throw Error(SSW_ERR_BAD_DIMS, "Reader::new_impl");
        ssw_config c = config.c();
        check(ssw_reader_create_rgb8(ctx.get(), image.data.data(), w_, h_, is_base ? 1 : 0, &c, &rd_), "Reader::new_impl");
    }
    Reader(Context& ctx, const ImageRgb16& image, bool is_base, const ReadConfig& config)
        : w_(image.width), h_(image.height) {
        if (image.data.size() != w_ * h_ * 3) throw Error(SSW_ERR_BAD_DIMS, "Reader::new_impl");
        ssw_config c = config.c();
        check(ssw_reader_create_rgb16(ctx.get(), image.data.data(), w_, h_, is_base ? 1 : 0, &c, &rd_), "Reader::new_impl");
    }
    size_t w_, h_;
    ssw_reader* rd_ = nullptr;
};

class ReaderDerived {                                  // algorithm.rs:448-456
public:
    ReaderDerived(Context& ctx, const ImageRgb32F& image, ssw_precision precision = SSW_PRECISION_F64)
        : r_(ctx, image, false, [&] { ReadConfig c; c.precision = precision; return c; }()) {}
    ReaderDerived(Context& ctx, const ImageRgb8& image, ssw_precision precision = SSW_PRECISION_F64)
        : r_(ctx, image, false, [&] { ReadConfig c; c.precision = precision; return c; }()) {}
    ReaderDerived(Context& ctx, const ImageRgb16& image, ssw_precision precision = SSW_PRECISION_F64)
        : r_(ctx, image, false, [&] { ReadConfig c; c.precision = precision; return c; }()) {}
    std::vector<float> coefficients() const { return r_.coefficients(); }

private:
    friend class Reader;
    Reader r_;
};

inline void Reader::extract(const ReaderDerived& derived, std::vector<float>& extracted) const {
    check(ssw_reader_extract(rd_, derived.r_.rd_, extracted.data(), extracted.size()), "Reader::extract");
}

struct Similarity {                                    // algorithm.rs:669-680
    float similarity;
    bool exceeds_sigma(float n_sigma) const { return similarity > n_sigma; }
};

class Tester {                                         // algorithm.rs:683-715
public:
    Tester(Context& ctx, const std::vector<float>& extracted_watermark) : ctx_(ctx), e_(extracted_watermark) {}
    Similarity similarity(const MarkBuf& comparison_watermark) const {
        float out = 0.f;
        check(ssw_similarity(ctx_.get(), e_.data(), e_.size(), comparison_watermark.data().data(),
                             comparison_watermark.data().size(), &out), "Tester::similarity");
        return {out};
    }

private:
    Context& ctx_;
    const std::vector<float>& e_;
};

// The callers' loops over host images (examples/main.rs:271-278, :383-415) as one streaming call each: uploads,
// kernels and downloads of consecutive groups of images overlap (ssw_batch_embed_host_rgb8 / ssw_batch_extract_host_rgb8).
// marks[i] is embedded into images[i]; all marks have one length.  Bit-identical to a loop over Writer / Reader.
inline std::vector<ImageRgb8> mark_many(Context& ctx, const std::vector<const ImageRgb8*>& images, const std::vector<const MarkBuf*>& marks,
                                        const WriteConfig& config = WriteConfig()) {
    if (images.empty() || images.size() != marks.size()) throw Error(SSW_ERR_BAD_ARG, "mark_many");
    const size_t w = images[0]->width, h = images[0]->height, k = marks[0]->data().size();
    std::vector<const uint8_t*> in(images.size());
    std::vector<float> m(images.size() * k);
    std::vector<ImageRgb8> out(images.size(), ImageRgb8(w, h));
    std::vector<uint8_t*> op(images.size());
    for (size_t i = 0; i < images.size(); ++i) {
        if (images[i]->width != w || images[i]->height != h || images[i]->data.size() != w * h * 3) throw Error(SSW_ERR_BAD_DIMS, "mark_many");
        if (marks[i]->data().size() != k) throw Error(SSW_ERR_LENGTH_MISMATCH, "mark_many");
        in[i] = images[i]->data.data();
        std::copy(marks[i]->data().begin(), marks[i]->data().end(), m.begin() + i * k);
        op[i] = out[i].data.data();
    }
    ssw_config c = config.c();
    check(ssw_batch_embed_host_rgb8(ctx.get(), &c, in.data(), in.size(), w, h, m.data(), k, op.data()), "mark_many");
    return out;
}
struct ExtractedMany { std::vector<std::vector<float>> extracted; std::vector<float> similarity; };
inline ExtractedMany extract_many(Context& ctx, const std::vector<const ImageRgb8*>& base, const std::vector<const ImageRgb8*>& derived,
                                  size_t k, const std::vector<const MarkBuf*>& marks, const ReadConfig& config = ReadConfig()) {
    if (base.empty() || base.size() != derived.size() || (!marks.empty() && marks.size() != base.size())) throw Error(SSW_ERR_BAD_ARG, "extract_many");
    const size_t n = base.size(), w = base[0]->width, h = base[0]->height;
    std::vector<const uint8_t*> bp(n), dp(n);
    std::vector<float> m(marks.empty() ? 0 : n * k), ext(n * k), sims(marks.empty() ? 0 : n);
    for (size_t i = 0; i < n; ++i) {
        if (base[i]->width != w || base[i]->height != h || derived[i]->width != w || derived[i]->height != h ||
            base[i]->data.size() != w * h * 3 || derived[i]->data.size() != w * h * 3)
            throw Error(SSW_ERR_BAD_DIMS, "extract_many");
        bp[i] = base[i]->data.data(); dp[i] = derived[i]->data.data();
        if (!marks.empty()) {
            if (marks[i]->data().size() != k) throw Error(SSW_ERR_LENGTH_MISMATCH, "extract_many");
            std::copy(marks[i]->data().begin(), marks[i]->data().end(), m.begin() + i * k);
        }
    }
    ssw_config c = config.c();
    check(ssw_batch_extract_host_rgb8(ctx.get(), &c, bp.data(), dp.data(), n, w, h, k, ext.data(), marks.empty() ? nullptr : m.data(),
                                      marks.empty() ? nullptr : sims.data()), "extract_many");
    ExtractedMany r;
    for (size_t i = 0; i < n; ++i) r.extracted.emplace_back(ext.begin() + i * k, ext.begin() + (i + 1) * k);
    r.similarity = sims;
    return r;
}

}  // namespace wm
