// Runs every public function, constructor and method of namespace wm (include/ssw.hpp) against the contract stub
// tests/cpp/ssw_stub.cpp, which is linked instead of libssw_hip.so: no HIP, no GPU.  Built with ASan + UBSan and without by
// tests/test_cpp_wrappers_cpu.py.  The stub reads every byte a call's contract reads and writes position patterns, so this
// program checks that each value arrives in the right slot of the right result object; then every flow is run again with
// the n-th library call failing, for every n, and must throw that status and leave no device block, pinned block, context,
// writer or reader alive.  Prints "ok".
//
// Coverage: flow -> the public names of namespace wm it runs (checked against ssw.hpp by tests/test_cpp_wrappers_cpu.py)
//   basics     Error::Error Error::status check Insertion::Option1 Insertion::Option2 Insertion::Option3 Insertion::Custom
//              WriteConfig::c ReadConfig::c ImageRgb32F::ImageRgb32F ImageRgb8::ImageRgb8 ImageRgba8::ImageRgba8
//              ImageRgb16::ImageRgb16 MarkBuf::MarkBuf MarkBuf::generate_normal MarkBuf::from MarkBuf::data MarkBuf::set_data
//              Placement::whole_frame Suspect::Suspect Quality::psnr Quality::psnr_luma Quality::changed_fraction Ssim::mean
//              Ssim::worst_value FilterJob::blur FilterJob::unsharp FilterJob::median Scale::by Similarity::exceeds_sigma
//   context    Context::Context Context::get Context::synchronize Context::set_stream Context::wait_event Context::record_event
//              Context::set_chunk_frames Context::pass_frames Context::set_overlap Context::set_prune Context::set_odd_split
//              Context::set_copy_threads Context::transfer_stats PinnedBuffer::PinnedBuffer PinnedBuffer::data PinnedBuffer::size
//   writer     Writer::Writer Writer::coefficient_image Writer::embed Writer::result Writer::mark Writer::mark_rgb8
//              Writer::mark_copies Writer::mark_copies_rgb8                                  (x ImageRgb32F, ImageRgb8, ImageRgb16)
//   reader     Reader::base Reader::Reader Reader::coefficients Reader::indices Reader::extract ReaderDerived::ReaderDerived
//              ReaderDerived::coefficients Tester::Tester Tester::similarity               (x ImageRgb32F, ImageRgb8, ImageRgb16)
//   trace      Reader::trace (both overloads; zero suspects, zero marks)
//   locate     locate (with and without sizes) locate_scaled
//   catalogue  signature Catalogue::Catalogue Catalogue::size Catalogue::name Catalogue::add Catalogue::match
//   strength   quality ssim collude jpeg filter resample scale_attack
//   rotation   rotation_matrix affine rotate Rotate::job rotate_attack unrotate
//   many       mark_many extract_many (with and without marks)
// End of coverage
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>

#include "ssw.hpp"

extern "C" {
void ssw_stub_fail_at(size_t n, int status);
size_t ssw_stub_calls(void);
void ssw_stub_live(size_t out[5]);
double ssw_stub_last(size_t i);
}

#define REQUIRE(c)                                                                   \
    do {                                                                             \
        if (!(c)) {                                                                  \
            std::fprintf(stderr, "%s:%d: REQUIRE(%s)\n", __FILE__, __LINE__, #c);   \
            std::exit(1);                                                            \
        }                                                                            \
    } while (0)

namespace {
constexpr size_t W = 12, H = 8, W2 = 16, H2 = 12, K = 5;

template <class Img> Img image(size_t w, size_t h, unsigned seed) {
    Img im(w, h);
    for (size_t i = 0; i < im.data.size(); ++i) im.data[i] = (typename decltype(im.data)::value_type)((i * 7 + seed) % 251);
    return im;
}
wm::MarkBuf mark(size_t k, float first) {
    std::vector<float> v(k);
    for (size_t i = 0; i < k; ++i) v[i] = first + (float)i;
    return wm::MarkBuf::from(v);
}
template <class T> bool all_bytes(const std::vector<T>& v, uint8_t b) {
    const uint8_t* p = reinterpret_cast<const uint8_t*>(v.data());
    for (size_t i = 0; i < v.size() * sizeof(T); ++i) if (p[i] != b) return false;
    return !v.empty();
}
template <class T> bool all_values(const std::vector<T>& v, T x) {
    for (const T& e : v) if (e != x) return false;
    return !v.empty();
}
bool frames_are(const std::vector<wm::ImageRgb8>& f, size_t n, size_t w, size_t h) {   // frame j: every byte j + 1
    if (f.size() != n) return false;
    for (size_t j = 0; j < n; ++j)
        if (f[j].width != w || f[j].height != h || f[j].data.size() != w * h * 3 || !all_bytes(f[j].data, (uint8_t)(j + 1))) return false;
    return true;
}
template <class F> int status_of(F f) {
    try { f(); } catch (const wm::Error& e) { return e.status(); }
    return SSW_OK;
}
bool nothing_live() {
    size_t live[5];
    ssw_stub_live(live);
    return live[0] + live[1] + live[2] + live[3] + live[4] == 0;
}
void trace_is(const wm::TraceResult& r, size_t n, size_t nm, size_t k) {
    REQUIRE(r.extracted.size() == n && r.sims.size() == n && r.best.size() == n && r.best_sim.size() == n && r.n_exceed.size() == n);
    for (size_t s = 0; s < n; ++s) {
        REQUIRE(r.extracted[s].size() == k && r.sims[s].size() == nm);
        for (size_t j = 0; j < k; ++j) REQUIRE(r.extracted[s][j] == (float)(1000 * s + j));
        for (size_t m = 0; m < nm; ++m) REQUIRE(r.sims[s][m] == (float)(100 * s + m));
        if (nm) REQUIRE(r.best[s] == s && r.best_sim[s] == (float)s + 0.5f && r.n_exceed[s] == s + 2);
        else REQUIRE(r.best[s] == wm::TraceResult::none && std::isnan(r.best_sim[s]) && r.n_exceed[s] == 0);
    }
}
const wm::WriteConfig WCFG{wm::Insertion::Option1(0.25f), wm::OrderingMethod::Legacy, SSW_PRECISION_F32};
const wm::ReadConfig RCFG{wm::Extraction::Option3(0.5f), wm::OrderingMethod::EnergyOrthogonal, SSW_PRECISION_F32};

// ---- no library call at all -------------------------------------------------------------------------------------------------
void basics() {
    const wm::Error e(SSW_ERR_K_TOO_LARGE, "here");
    REQUIRE(e.status() == SSW_ERR_K_TOO_LARGE && std::string(e.what()).find("here: ") == 0);
    REQUIRE(std::string(wm::Error(SSW_ERR_HIP, "x").what()).find("[stub]") != std::string::npos);
    wm::check(SSW_OK, "fine");
    REQUIRE(status_of([] { wm::check(SSW_ERR_NOT_BASE, "x"); }) == SSW_ERR_NOT_BASE);
    REQUIRE(wm::Insertion::Option1(1.f).method == SSW_OPTION1 && wm::Insertion::Option2(2.f).method == SSW_OPTION2 && wm::Insertion::Option2(2.f).alpha == 2.f);
    REQUIRE(wm::Insertion::Option3(3.f).method == SSW_OPTION3 && wm::Insertion::Custom().method == SSW_METHOD_CUSTOM);
    const ssw_config wc = WCFG.c(), rc = RCFG.c(), dw = wm::WriteConfig().c(), dr = wm::ReadConfig().c();
    REQUIRE(wc.ordering == SSW_ORDER_LEGACY && wc.method == SSW_OPTION1 && wc.alpha == 0.25f && wc.precision == SSW_PRECISION_F32);
    REQUIRE(rc.ordering == SSW_ORDER_ENERGY_ORTHOGONAL && rc.method == SSW_OPTION3 && rc.alpha == 0.5f && rc.precision == SSW_PRECISION_F32);
    REQUIRE(dw.ordering == SSW_ORDER_ENERGY && dw.method == SSW_OPTION2 && dw.alpha == 0.1f && dw.precision == SSW_PRECISION_F64);
    REQUIRE(dr.ordering == SSW_ORDER_ENERGY && dr.method == SSW_OPTION2 && dr.alpha == 0.1f && dr.precision == SSW_PRECISION_F64);
    REQUIRE(wm::ImageRgb32F().data.empty() && wm::ImageRgb8().data.empty() && wm::ImageRgba8().data.empty() && wm::ImageRgb16().data.empty());
    REQUIRE(wm::ImageRgb32F(W, H).data.size() == W * H * 3 && wm::ImageRgb8(W, H).data.size() == W * H * 3);
    REQUIRE(wm::ImageRgba8(W, H).data.size() == W * H * 4 && wm::ImageRgb16(W, H).data.size() == W * H * 3 && wm::ImageRgb16(W, H).width == W);
    wm::MarkBuf m = wm::MarkBuf();
    REQUIRE(m.data().empty() && wm::MarkBuf::generate_normal(K).data().size() == K);
    const float v[3] = {1.f, 2.f, 3.f};
    m.set_data(v, 3);
    REQUIRE(m.data() == std::vector<float>({1.f, 2.f, 3.f}) && wm::MarkBuf::from(v, 2).data() == std::vector<float>({1.f, 2.f}));
    REQUIRE(wm::MarkBuf::from(std::vector<float>{4.f}).data() == std::vector<float>{4.f});
    const wm::ImageRgb8 im = image<wm::ImageRgb8>(W, H, 1);
    const wm::ImageRgba8 ima = image<wm::ImageRgba8>(W2, H2, 2);
    const wm::Placement whole = wm::Placement::whole_frame(im);
    REQUIRE(whole.x == 0 && whole.y == 0 && whole.w == W && whole.h == H);
    const wm::Suspect s3 = wm::Suspect(im), s4 = wm::Suspect(ima);
    REQUIRE(s3.data == im.data.data() && s3.width == W && s3.height == H && s3.channels == 3);
    REQUIRE(s4.data == ima.data.data() && s4.width == W2 && s4.height == H2 && s4.channels == 4);
    wm::Quality q;
    REQUIRE(std::isinf(q.psnr()) && std::isinf(q.psnr_luma()) && q.changed_fraction() == 0.0);
    q.sse[0] = 10; q.sse[1] = 20; q.sse[2] = 30; q.sse_luma = 50; q.changed = 6; q.pixels = 4;
    REQUIRE(q.psnr() == 10.0 * std::log10(255.0 * 255.0 * 3.0 * 4.0 / 60.0) && q.psnr_luma() == 10.0 * std::log10(255.0 * 255.0 * 4.0 / 50.0));
    REQUIRE(q.changed_fraction() == 0.5);
    wm::Ssim ss;
    REQUIRE(ss.mean() == 0.0);
    ss.sum = (int64_t)SSW_SSIM_ONE * 3; ss.windows = 4; ss.worst = SSW_SSIM_ONE / 2;
    REQUIRE(ss.mean() == 0.75 && ss.worst_value() == 0.5);
    const wm::FilterJob b = wm::FilterJob::blur(2, 1.5f), u = wm::FilterJob::unsharp(1), md = wm::FilterJob::median(3);
    REQUIRE(b.frame == 2 && b.kind == SSW_FILTER_BLUR && b.radius == 1.5f && b.percent == 0 && b.threshold == 0);
    REQUIRE(u.frame == 1 && u.kind == SSW_FILTER_UNSHARP && u.radius == 2.0f && u.percent == 150 && u.threshold == 3);
    REQUIRE(md.frame == 3 && md.kind == SSW_FILTER_MEDIAN3 && md.radius == 0.0f && md.percent == 0 && md.threshold == 0);
    const wm::Scale sc = wm::Scale::by(1, 10, 7, 0.5, wm::ResampleFilter::Box), tiny = wm::Scale::by(0, 10, 7, 0.01);
    REQUIRE(sc.frame == 1 && sc.nw == 5 && sc.nh == 4 && sc.filter == wm::ResampleFilter::Box && tiny.nw == 1 && tiny.nh == 1);
    REQUIRE(wm::Similarity{6.5f}.exceeds_sigma(6.0f) && !wm::Similarity{6.0f}.exceeds_sigma(6.0f));
    // what the header checks itself, before any library call
    wm::ImageRgb8 bad8(W, H);
    bad8.data.pop_back();
    wm::ImageRgba8 bada(W, H);
    bada.data.pop_back();
    REQUIRE(status_of([&] { (void)wm::Suspect(bad8); }) == SSW_ERR_BAD_DIMS && status_of([&] { (void)wm::Suspect(bada); }) == SSW_ERR_BAD_DIMS);
}

// ---- the flows: each makes its own context, so that the sweep fails that call too --------------------------------------------------
void context() {
    wm::Context ctx(3);
    REQUIRE(ctx.get() != nullptr && ssw_stub_last(0) == 3);
    ctx.synchronize();
    int stream = 0, event = 0;
    ctx.set_stream(&stream);
    REQUIRE(ssw_stub_last(0) == (double)(uintptr_t)&stream);
    ctx.set_stream(nullptr);
    REQUIRE(ssw_stub_last(0) == 0);
    ctx.wait_event(&event);
    REQUIRE(ssw_stub_last(0) == (double)(uintptr_t)&event);
    ctx.record_event(&event);
    REQUIRE(ssw_stub_last(0) == (double)(uintptr_t)&event);
    ctx.set_chunk_frames(7);
    REQUIRE(ssw_stub_last(0) == 7);
    REQUIRE(ctx.pass_frames(3, W, H) == 3 * 1000000 + W * 1000 + H);
    ctx.set_overlap(true);
    REQUIRE(ssw_stub_last(0) == 1);
    ctx.set_overlap(false);
    REQUIRE(ssw_stub_last(0) == 0);
    ctx.set_prune(true);
    REQUIRE(ssw_stub_last(0) == 1);
    ctx.set_prune(false);
    REQUIRE(ssw_stub_last(0) == 0);
    ctx.set_odd_split(true);
    REQUIRE(ssw_stub_last(0) == 1);
    ctx.set_odd_split(false);
    REQUIRE(ssw_stub_last(0) == 0);
    ctx.set_copy_threads(3);
    REQUIRE(ssw_stub_last(0) == 3);
    REQUIRE(ctx.transfer_stats(true) == std::vector<double>({1, 2, 3, 4, 5, 6}) && ssw_stub_last(0) == 1);
    REQUIRE(ctx.transfer_stats().size() == SSW_TRANSFER_STAT_COUNT && ssw_stub_last(0) == 0);
    wm::PinnedBuffer pinned(ctx, 40);
    REQUIRE(pinned.size() == 40 && pinned.data() != nullptr);
    std::memset(pinned.data(), 0x5A, pinned.size());
    size_t live[5];
    ssw_stub_live(live);
    REQUIRE(live[1] == 1 && live[2] == 1);
}

template <class Img> void writer() {
    wm::Context ctx;
    const Img im = image<Img>(W, H, 3);
    const wm::MarkBuf m0 = mark(K, 1.f), m1 = mark(K + 2, 2.f), m2 = mark(K, 3.f), m3 = mark(K, 4.f);
    {
        wm::Writer w(ctx, im, WCFG);
        REQUIRE(ssw_stub_last(0) == sizeof(im.data[0]) && ssw_stub_last(1) == W && ssw_stub_last(2) == H && ssw_stub_last(3) == SSW_ORDER_LEGACY);
        REQUIRE(ssw_stub_last(4) == SSW_OPTION1 && ssw_stub_last(5) == 0.25 && ssw_stub_last(6) == SSW_PRECISION_F32);
        const std::vector<float> coef = w.coefficient_image();
        REQUIRE(coef.size() == W * H);
        for (size_t j = 0; j < coef.size(); ++j) REQUIRE(coef[j] == (float)j);
        w.embed({&m0, &m1});
        REQUIRE(ssw_stub_last(0) == 2 && ssw_stub_last(1) == K);
        const wm::ImageRgb32F out = w.result();
        REQUIRE(out.width == W && out.height == H && out.data.size() == W * H * 3 && all_bytes(out.data, 1));
    }
    {
        wm::Writer w(ctx, im);
        REQUIRE(ssw_stub_last(3) == SSW_ORDER_ENERGY && ssw_stub_last(6) == SSW_PRECISION_F64);
        const wm::ImageRgb32F out = w.mark({&m0});
        REQUIRE(out.width == W && out.height == H && all_bytes(out.data, 1));
    }
    {
        wm::Writer w(ctx, im);
        const wm::ImageRgb8 out = w.mark_rgb8({&m1});
        REQUIRE(ssw_stub_last(0) == 1 && ssw_stub_last(1) == K + 2);
        REQUIRE(out.width == W && out.height == H && out.data.size() == W * H * 3 && all_bytes(out.data, 1));
    }
    wm::Writer w(ctx, im);
    const std::vector<wm::ImageRgb32F> c32 = w.mark_copies({&m0, &m2, &m3});
    REQUIRE(ssw_stub_last(0) == 3 && ssw_stub_last(1) == K && c32.size() == 3);
    for (size_t i = 0; i < 3; ++i) REQUIRE(c32[i].width == W && c32[i].height == H && c32[i].data.size() == W * H * 3 && all_values(c32[i].data, (float)(i + 1)));
    const std::vector<wm::ImageRgb8> c8 = w.mark_copies_rgb8({&m0, &m2, &m3});
    REQUIRE(frames_are(c8, 3, W, H));
    REQUIRE(w.mark_copies({}).empty() && w.mark_copies_rgb8({}).empty());
}

template <class Img> void reader() {
    wm::Context ctx;
    const Img im = image<Img>(W, H, 4), other = image<Img>(W, H, 5);
    wm::Reader base = wm::Reader::base(ctx, im, RCFG);
    REQUIRE(ssw_stub_last(0) == sizeof(im.data[0]) && ssw_stub_last(1) == W && ssw_stub_last(2) == H && ssw_stub_last(3) == SSW_ORDER_ENERGY_ORTHOGONAL);
    REQUIRE(ssw_stub_last(4) == SSW_OPTION3 && ssw_stub_last(5) == 0.5 && ssw_stub_last(6) == SSW_PRECISION_F32 && ssw_stub_last(7) == 1);
    wm::Reader moved = wm::Reader(std::move(base));                      // the moved-from reader destroys nothing
    wm::Reader plain = wm::Reader::base(ctx, im);
    REQUIRE(ssw_stub_last(3) == SSW_ORDER_ENERGY && ssw_stub_last(6) == SSW_PRECISION_F64);
    const std::vector<float> coef = moved.coefficients();
    REQUIRE(coef.size() == W * H);
    for (size_t j = 0; j < coef.size(); ++j) REQUIRE(coef[j] == (float)j);
    REQUIRE(moved.indices(K) == std::vector<uint64_t>({0, 1, 2, 3, 4}) && moved.indices(0).empty());
    wm::ReaderDerived derived(ctx, other, SSW_PRECISION_F32);
    REQUIRE(ssw_stub_last(6) == SSW_PRECISION_F32 && ssw_stub_last(7) == 0);
    wm::ReaderDerived canonical(ctx, other);
    REQUIRE(ssw_stub_last(6) == SSW_PRECISION_F64 && ssw_stub_last(7) == 0);
    REQUIRE(derived.coefficients().size() == W * H && canonical.coefficients()[W * H - 1] == (float)(W * H - 1));
    std::vector<float> ext(K, -1.f);
    moved.extract(derived, ext);
    for (size_t j = 0; j < K; ++j) REQUIRE(ext[j] == (float)j + 0.5f);
    const wm::Tester tester(ctx, ext);
    const wm::Similarity sim = tester.similarity(mark(K, 1.f));
    REQUIRE(sim.similarity == (float)K + 0.25f && sim.exceeds_sigma(5.0f) && !sim.exceeds_sigma(6.0f));
}

void trace() {
    wm::Context ctx;
    const wm::ImageRgb8 original = image<wm::ImageRgb8>(W, H, 6), s0 = image<wm::ImageRgb8>(W, H, 7), s1 = image<wm::ImageRgb8>(W, H, 8);
    const wm::MarkBuf m0 = mark(K, 1.f), m1 = mark(K, 2.f), m2 = mark(K, 3.f);
    const wm::Reader base = wm::Reader::base(ctx, original);
    trace_is(base.trace({&s0, &s1}, {&m0, &m1, &m2}, 4.5f), 2, 3, K);
    REQUIRE(ssw_stub_last(0) == 2 && ssw_stub_last(1) == K && ssw_stub_last(2) == 3 && ssw_stub_last(3) == 4.5);
    trace_is(base.trace({&s0, &s1}, {&m0, &m1, &m2}), 2, 3, K);
    REQUIRE(ssw_stub_last(3) == 6.0);
    trace_is(base.trace({}, {&m0, &m1, &m2}), 0, 3, K);                   // zero suspects
    trace_is(base.trace({&s0, &s1}, {}), 2, 0, 0);                        // zero marks: nothing to extract against
    // restoring trace: a copy as it is, a smaller copy of the whole frame, an RGBA cut-out
    const wm::ImageRgb8 small = image<wm::ImageRgb8>(6, 4, 9);
    const wm::ImageRgba8 cut = image<wm::ImageRgba8>(5, 3, 10);
    const std::vector<wm::Suspect> suspects{s0, small, cut};
    const std::vector<wm::Placement> placements{wm::Placement::whole_frame(original), wm::Placement::whole_frame(original), wm::Placement{2, 1, 0, 0}};
    trace_is(base.trace(original, suspects, placements, {&m0, &m1, &m2}, 3.5f), 3, 3, K);
    const double expected[3][7] = {{W, H, 3, 0, 0, W, H}, {6, 4, 3, 0, 0, W, H}, {5, 3, 4, 2, 1, 0, 0}};
    REQUIRE(ssw_stub_last(0) == 3 && ssw_stub_last(1) == K && ssw_stub_last(2) == 3 && ssw_stub_last(3) == 3.5);
    for (size_t s = 0; s < 3; ++s)
        for (size_t f = 0; f < 7; ++f) REQUIRE(ssw_stub_last(4 + 7 * s + f) == expected[s][f]);
    trace_is(base.trace(original, suspects, placements, {&m0, &m1}), 3, 2, K);      // suspects != marks
    REQUIRE(ssw_stub_last(2) == 2 && ssw_stub_last(3) == 6.0);
    trace_is(base.trace(original, {}, {}, {&m0}), 0, 1, K);
    trace_is(base.trace(original, suspects, placements, {}), 3, 0, 0);
}

const size_t LW = 100, LH = 90;      // the frame of the locate and signature flows: a scale ladder starts at 32 pixels
struct Cuts {
    wm::ImageRgb8 a = image<wm::ImageRgb8>(40, 36, 11), c = image<wm::ImageRgb8>(33, 37, 13);
    wm::ImageRgba8 b = image<wm::ImageRgba8>(50, 41, 12);
    std::vector<wm::Suspect> suspects() const { return {a, b, c}; }
};
void locate() {
    wm::Context ctx;
    const wm::ImageRgb8 original = image<wm::ImageRgb8>(LW, LH, 14);
    const Cuts cuts;
    const std::vector<wm::Suspect> suspects = cuts.suspects();
    const std::vector<wm::Located> own = wm::locate(ctx, original, suspects);
    REQUIRE(own.size() == 3 && ssw_stub_last(0) == LW && ssw_stub_last(1) == LH && ssw_stub_last(2) == 3);
    const std::vector<wm::Located> sized = wm::locate(ctx, original, suspects, {wm::Placement{9, 9, 80, 72}, wm::Placement{}, wm::Placement{0, 0, 30, 20}});
    const size_t own_w[3] = {40, 50, 33}, own_h[3] = {36, 41, 37}, sized_w[3] = {80, 50, 30}, sized_h[3] = {72, 41, 20};
    for (size_t i = 0; i < 3; ++i) {
        REQUIRE(own[i].placement.x == 10 + i && own[i].placement.y == 20 + i && own[i].placement.w == own_w[i] && own[i].placement.h == own_h[i]);
        REQUIRE(own[i].sad == 1000 + i && own[i].mean_abs_diff == (double)(1000 + i) / ((double)own_w[i] * (double)own_h[i]));
        REQUIRE(sized[i].placement.x == 10 + i && sized[i].placement.y == 20 + i && sized[i].placement.w == sized_w[i] && sized[i].placement.h == sized_h[i]);
        REQUIRE(sized[i].sad == 1000 + i && sized[i].mean_abs_diff == (double)(1000 + i) / ((double)sized_w[i] * (double)sized_h[i]));
    }
    REQUIRE(wm::locate(ctx, original, {}).empty());
    size_t live[5];
    ssw_stub_live(live);
    REQUIRE(live[0] == 0);
}
void locate_scaled() {
    wm::Context ctx;
    const wm::ImageRgb8 original = image<wm::ImageRgb8>(LW, LH, 15);
    const Cuts cuts;
    const std::vector<wm::Located> found = wm::locate_scaled(ctx, original, cuts.suspects(), {wm::ScaleRange{40, 80}, wm::ScaleRange{41, 81}, wm::ScaleRange{42, 82}});
    const size_t sw[3] = {40, 50, 33}, sh[3] = {36, 41, 37};
    REQUIRE(found.size() == 3 && ssw_stub_last(0) == LW && ssw_stub_last(1) == LH && ssw_stub_last(2) == 3);
    for (size_t i = 0; i < 3; ++i) {
        const size_t pw = 64 + 8 * i, ph = (2 * sh[i] * pw + sw[i]) / (2 * sw[i]);
        REQUIRE(ssw_stub_last(3 + 2 * i) == 40 + i && ssw_stub_last(4 + 2 * i) == 80 + i);
        REQUIRE(found[i].placement.x == 10 + i && found[i].placement.y == 20 + i && found[i].placement.w == pw && found[i].placement.h == ph);
        REQUIRE(found[i].sad == 1000 + i && found[i].mean_abs_diff == (double)(1000 + i) / ((double)pw * (double)ph));
    }
    REQUIRE(wm::locate_scaled(ctx, original, {}, {}).empty());
    size_t live[5];
    ssw_stub_live(live);
    REQUIRE(live[0] == 0);
}

void catalogue() {
    wm::Context ctx;
    const Cuts cuts;
    const std::vector<std::array<uint8_t, 1024>> sigs = wm::signature(ctx, cuts.suspects());
    REQUIRE(sigs.size() == 3);
    for (size_t i = 0; i < 3; ++i)
        for (uint8_t v : sigs[i]) REQUIRE((size_t)v == i + 1);
    REQUIRE(wm::signature(ctx, {}).empty());
    wm::Catalogue cat(ctx);
    REQUIRE(cat.size() == 0);
    const auto is = [](const std::vector<std::vector<wm::Catalogue::Match>>& m, size_t nq, size_t top, size_t nc) {
        REQUIRE(m.size() == nq);
        for (size_t s = 0; s < nq; ++s) {
            REQUIRE(m[s].size() == top);
            for (size_t t = 0; t < top; ++t) {
                if (t < nc) REQUIRE(m[s][t].index == 8 * s + t && m[s][t].distance == 100 * s + t);
                else REQUIRE(m[s][t].index == wm::Catalogue::Match::none && m[s][t].distance == wm::Catalogue::Match::none);
            }
        }
    };
    is(cat.match(cuts.suspects(), 2), 3, 2, 0);                            // an empty catalogue
    cat.add("a", cuts.a);
    cat.add("b", cuts.b);
    REQUIRE(cat.size() == 2 && cat.name(0) == "a" && cat.name(1) == "b");
    is(cat.match({}, 4), 0, 4, 2);                                         // no suspects
    is(cat.match(cuts.suspects()), 3, 1, 2);
    REQUIRE(ssw_stub_last(0) == 3 && ssw_stub_last(1) == 2 && ssw_stub_last(2) == 1);
    is(cat.match(cuts.suspects(), 8), 3, 8, 2);
    size_t live[5];
    ssw_stub_live(live);
    REQUIRE(live[0] == 1);                                                 // the resident signatures and nothing else
    cat.add("c", cuts.c);
    is(cat.match({cuts.b, cuts.a}, 8), 2, 8, 3);                           // uploads the three again: the stub reads nc * 1024 bytes
    REQUIRE(ssw_stub_last(0) == 2 && ssw_stub_last(1) == 3 && ssw_stub_last(2) == 8 && cat.size() == 3 && cat.name(2) == "c");
    ssw_stub_live(live);
    REQUIRE(live[0] == 1);
}

void strength() {
    wm::Context ctx;
    const wm::ImageRgb8 original = image<wm::ImageRgb8>(W2, H2, 16), c0 = image<wm::ImageRgb8>(W2, H2, 17), c1 = image<wm::ImageRgb8>(W2, H2, 18),
                        c2 = image<wm::ImageRgb8>(W2, H2, 19);
    const std::vector<const wm::ImageRgb8*> two{&c0, &c1}, three{&c0, &c1, &c2};
    const std::vector<wm::Quality> q = wm::quality(ctx, original, two);
    REQUIRE(q.size() == 2 && ssw_stub_last(0) == 1 && ssw_stub_last(1) == 2 && ssw_stub_last(2) == W2 && ssw_stub_last(3) == H2);
    for (size_t i = 0; i < 2; ++i)
        REQUIRE(q[i].sse[0] == 16 * i && q[i].sse[1] == 16 * i + 1 && q[i].sse[2] == 16 * i + 2 && q[i].sse_luma == 16 * i + 3 && q[i].changed == 16 * i + 4 &&
                q[i].max_abs == 16 * i + 5 && q[i].pixels == W2 * H2);
    REQUIRE(wm::quality(ctx, original, {}).empty());
    const std::vector<wm::Ssim> s = wm::ssim(ctx, original, two);
    const size_t nx = W2 / 4 - 1, ny = H2 / 4 - 1;
    REQUIRE(s.size() == 2);
    for (size_t i = 0; i < 2; ++i)      // word 0 = 16 i, word 1 = 16 i + 1: a key whose upper half is 0 and whose index is 16 i + 1
        REQUIRE(s[i].sum == (int64_t)(16 * i) && s[i].worst == -SSW_SSIM_ONE && s[i].worst_x == (16 * i + 1) % nx * 4 && s[i].worst_y == (16 * i + 1) / nx * 4 &&
                s[i].windows == nx * ny);
    REQUIRE(frames_are(wm::collude(ctx, three, {{SSW_COLLUDE_MEDIAN, {0, 1}}, {SSW_COLLUDE_MOSAIC, {1, 0, 2}}}), 2, W2, H2));
    REQUIRE(ssw_stub_last(0) == 3 && ssw_stub_last(3) == 2 && ssw_stub_last(4) == SSW_COLLUDE_MOSAIC && ssw_stub_last(5) == 3 && ssw_stub_last(6) == 2);
    REQUIRE(wm::collude(ctx, three, {}).empty());
    REQUIRE(frames_are(wm::jpeg(ctx, three, {{0, 75}, {2, 10}}), 2, W2, H2));
    REQUIRE(ssw_stub_last(0) == 3 && ssw_stub_last(1) == W2 && ssw_stub_last(2) == H2 && ssw_stub_last(4) == 2 && ssw_stub_last(5) == 10);
    REQUIRE(frames_are(wm::filter(ctx, three, {wm::FilterJob::blur(0, 1.5f), wm::FilterJob::median(1), wm::FilterJob::unsharp(2, 3.0f, 120, 4)}), 3, W2, H2));
    REQUIRE(ssw_stub_last(4) == 2 && ssw_stub_last(5) == SSW_FILTER_UNSHARP && ssw_stub_last(6) == 3.0 && ssw_stub_last(7) == 120 && ssw_stub_last(8) == 4);
    REQUIRE(frames_are(wm::resample(ctx, three, 5, 7, wm::ResampleFilter::Lanczos), 3, 5, 7));
    REQUIRE(ssw_stub_last(0) == 3 && ssw_stub_last(1) == W2 && ssw_stub_last(2) == H2 && ssw_stub_last(3) == 5 && ssw_stub_last(4) == 7 &&
            ssw_stub_last(5) == SSW_RESAMPLE_LANCZOS);
    REQUIRE(frames_are(wm::resample(ctx, three, 5, 7), 3, 5, 7) && ssw_stub_last(5) == SSW_RESAMPLE_BICUBIC);
    REQUIRE(frames_are(wm::scale_attack(ctx, three, {wm::Scale::by(1, W2, H2, 0.5), wm::Scale{2, 9, 5, wm::ResampleFilter::Bilinear}}), 2, W2, H2));
    REQUIRE(ssw_stub_last(3) == 2 && ssw_stub_last(4) == 2 && ssw_stub_last(5) == 9 && ssw_stub_last(6) == 5 && ssw_stub_last(7) == SSW_RESAMPLE_BILINEAR);
}

void rotation() {
    wm::Context ctx;
    const wm::ImageRgb8 original = image<wm::ImageRgb8>(W2, H2, 20), c0 = image<wm::ImageRgb8>(W2, H2, 21), c1 = image<wm::ImageRgb8>(W2, H2, 22),
                        c2 = image<wm::ImageRgb8>(W2, H2, 23);
    const std::vector<const wm::ImageRgb8*> three{&c0, &c1, &c2};
    REQUIRE(wm::rotation_matrix(1.5, W2, H2) == (wm::Matrix{1.5, (double)W2, (double)H2, 3, 4, 5}));
    const wm::Matrix m{1, 2, 3, 4, 5, 6};
    REQUIRE(frames_are(wm::affine(ctx, three, 7, 5, m, wm::AffineFilter::Bilinear, {9, 8, 7}), 3, 7, 5));
    const double affine_args[15] = {3, W2, H2, 7, 5, SSW_AFFINE_BILINEAR, 9, 8, 7, 1, 2, 3, 4, 5, 6};
    for (size_t i = 0; i < 15; ++i) REQUIRE(ssw_stub_last(i) == affine_args[i]);
    REQUIRE(frames_are(wm::affine(ctx, three, 7, 5, m), 3, 7, 5) && ssw_stub_last(5) == SSW_AFFINE_BICUBIC && ssw_stub_last(6) == 0);
    REQUIRE(frames_are(wm::rotate(ctx, three, 2.5, wm::AffineFilter::Bilinear, {1, 2, 3}), 3, W2, H2));
    const double rotate_args[15] = {3, W2, H2, W2, H2, SSW_AFFINE_BILINEAR, 1, 2, 3, 2.5, W2, H2, 3, 4, 5};
    for (size_t i = 0; i < 15; ++i) REQUIRE(ssw_stub_last(i) == rotate_args[i]);
    REQUIRE(frames_are(wm::rotate(ctx, three, 2.5), 3, W2, H2) && ssw_stub_last(5) == SSW_AFFINE_BICUBIC);
    const ssw_rotate_job j = wm::Rotate{2, 3.5, wm::AffineFilter::Bilinear, {{4, 5, 6}}}.job(W2, H2);
    REQUIRE(j.frame == 2 && j.filter == SSW_AFFINE_BILINEAR && j.fill[0] == 4 && j.fill[1] == 5 && j.fill[2] == 6 && j.fill[3] == 0);
    REQUIRE(j.forward[0] == 3.5 && j.forward[1] == W2 && j.forward[2] == H2 && j.forward[5] == 5 && j.back[0] == -3.5 && j.back[1] == W2 && j.back[5] == 5);
    REQUIRE(frames_are(wm::rotate_attack(ctx, original, three, {wm::Rotate{0, 1.0}, wm::Rotate{2, 3.5, wm::AffineFilter::Bilinear, {{4, 5, 6}}}}), 2, W2, H2));
    const double attack_args[15] = {3, W2, H2, 2, 2, SSW_AFFINE_BILINEAR, 4, 5, 6, 3.5, W2, H2, -3.5, W2, H2};
    for (size_t i = 0; i < 15; ++i) REQUIRE(ssw_stub_last(i) == attack_args[i]);
    REQUIRE(frames_are(wm::unrotate(ctx, original, three, {1.0, 2.0, 4.5}), 3, W2, H2));
    const double undo_args[15] = {3, W2, H2, 3, 2, SSW_AFFINE_BICUBIC, 0, 0, 0, 4.5, W2, H2, -4.5, W2, H2};
    for (size_t i = 0; i < 15; ++i) REQUIRE(ssw_stub_last(i) == undo_args[i]);
}

void many() {
    wm::Context ctx;
    const wm::ImageRgb8 a = image<wm::ImageRgb8>(W, H, 24), b = image<wm::ImageRgb8>(W, H, 25), c = image<wm::ImageRgb8>(W, H, 26);
    const wm::MarkBuf m0 = mark(K, 1.f), m1 = mark(K, 2.f), m2 = mark(K, 3.f);
    REQUIRE(frames_are(wm::mark_many(ctx, {&a, &b, &c}, {&m0, &m1, &m2}, WCFG), 3, W, H));
    const double embed_args[8] = {3, W, H, K, SSW_ORDER_LEGACY, SSW_OPTION1, 0.25, SSW_PRECISION_F32};
    for (size_t i = 0; i < 8; ++i) REQUIRE(ssw_stub_last(i) == embed_args[i]);
    REQUIRE(frames_are(wm::mark_many(ctx, {&a, &b}, {&m0, &m1}), 2, W, H) && ssw_stub_last(0) == 2 && ssw_stub_last(4) == SSW_ORDER_ENERGY);
    const auto is = [](const wm::ExtractedMany& r, size_t n, bool sims) {
        REQUIRE(r.extracted.size() == n && r.similarity.size() == (sims ? n : 0));
        for (size_t i = 0; i < n; ++i) {
            REQUIRE(r.extracted[i].size() == K && (!sims || r.similarity[i] == (float)i + 0.5f));
            for (size_t j = 0; j < K; ++j) REQUIRE(r.extracted[i][j] == (float)(1000 * i + j));
        }
    };
    is(wm::extract_many(ctx, {&a, &b, &c}, {&c, &a, &b}, K, {&m0, &m1, &m2}, RCFG), 3, true);
    const double extract_args[8] = {3, W, H, K, SSW_ORDER_ENERGY_ORTHOGONAL, SSW_OPTION3, 0.5, SSW_PRECISION_F32};
    for (size_t i = 0; i < 8; ++i) REQUIRE(ssw_stub_last(i) == extract_args[i]);
    is(wm::extract_many(ctx, {&a, &b}, {&c, &a}, K, {}), 2, false);
    REQUIRE(ssw_stub_last(0) == 2 && ssw_stub_last(4) == SSW_ORDER_ENERGY && ssw_stub_last(7) == SSW_PRECISION_F64);
}

// ---- every throw Error(...) of the header's own, with the status it names --------------------------------------------------------
void header_checks() {
    wm::Context ctx;
    wm::ImageRgb32F bad32(W, H);
    wm::ImageRgb8 bad8(W, H);
    wm::ImageRgb16 bad16(W, H);
    bad32.data.pop_back(); bad8.data.pop_back(); bad16.data.pop_back();
    const wm::ImageRgb8 good = image<wm::ImageRgb8>(W, H, 27), wide = image<wm::ImageRgb8>(W2, H2, 28), tiny = image<wm::ImageRgb8>(4, 4, 29);
    const wm::MarkBuf m0 = mark(K, 1.f), longer = mark(K + 1, 2.f);
    const size_t before = ssw_stub_calls();
    REQUIRE(status_of([&] { wm::Writer w(ctx, bad32); }) == SSW_ERR_BAD_DIMS && status_of([&] { wm::Writer w(ctx, bad8); }) == SSW_ERR_BAD_DIMS);
    REQUIRE(status_of([&] { wm::Writer w(ctx, bad16); }) == SSW_ERR_BAD_DIMS);
    REQUIRE(status_of([&] { wm::Reader::base(ctx, bad32); }) == SSW_ERR_BAD_DIMS && status_of([&] { wm::Reader::base(ctx, bad8); }) == SSW_ERR_BAD_DIMS);
    REQUIRE(status_of([&] { wm::Reader::base(ctx, bad16); }) == SSW_ERR_BAD_DIMS);
    REQUIRE(status_of([&] { wm::ReaderDerived d(ctx, bad32); }) == SSW_ERR_BAD_DIMS && status_of([&] { wm::ReaderDerived d(ctx, bad8); }) == SSW_ERR_BAD_DIMS);
    REQUIRE(status_of([&] { wm::ReaderDerived d(ctx, bad16); }) == SSW_ERR_BAD_DIMS);
    REQUIRE(ssw_stub_calls() == before);                                   // none of them reached the library
    wm::Writer w(ctx, good);
    REQUIRE(status_of([&] { w.mark_copies({&m0, &longer}); }) == SSW_ERR_LENGTH_MISMATCH);
    REQUIRE(status_of([&] { w.mark_copies_rgb8({&longer, &m0}); }) == SSW_ERR_LENGTH_MISMATCH);
    const wm::Reader base = wm::Reader::base(ctx, good);
    const size_t made = ssw_stub_calls();
    REQUIRE(status_of([&] { base.trace({&good, &wide}, {&m0}); }) == SSW_ERR_BAD_DIMS && status_of([&] { base.trace({&bad8}, {&m0}); }) == SSW_ERR_BAD_DIMS);
    REQUIRE(status_of([&] { base.trace({&good}, {&m0, &longer}); }) == SSW_ERR_LENGTH_MISMATCH);
    REQUIRE(status_of([&] { base.trace(good, {good}, {}, {&m0}); }) == SSW_ERR_BAD_DIMS);                         // placements.size() != n
    REQUIRE(status_of([&] { base.trace(wide, {good}, {wm::Placement{}}, {&m0}); }) == SSW_ERR_BAD_DIMS);          // not the reader's frame
    REQUIRE(status_of([&] { base.trace(bad8, {good}, {wm::Placement{}}, {&m0}); }) == SSW_ERR_BAD_DIMS);
    REQUIRE(status_of([&] { base.trace(good, {good}, {wm::Placement{}}, {&m0, &longer}); }) == SSW_ERR_LENGTH_MISMATCH);
    REQUIRE(status_of([&] { wm::locate(ctx, good, {good}, {wm::Placement{}, wm::Placement{}}); }) == SSW_ERR_BAD_DIMS);   // sizes.size() != n
    REQUIRE(status_of([&] { wm::locate(ctx, bad8, {good}); }) == SSW_ERR_BAD_DIMS);
    REQUIRE(status_of([&] { wm::locate_scaled(ctx, good, {good}, {}); }) == SSW_ERR_BAD_DIMS);                    // ranges.size() != n
    REQUIRE(status_of([&] { wm::locate_scaled(ctx, bad8, {good}, {wm::ScaleRange{32, 40}}); }) == SSW_ERR_BAD_DIMS);
    REQUIRE(status_of([&] { wm::ssim(ctx, tiny, {&tiny}); }) == SSW_ERR_BAD_ARG);
    REQUIRE(status_of([&] { wm::collude(ctx, {&good}, {{SSW_COLLUDE_MIN, {}}}); }) == SSW_ERR_BAD_ARG);
    REQUIRE(status_of([&] { wm::collude(ctx, {&good}, {{SSW_COLLUDE_MIN, std::vector<uint32_t>(17, 0)}}); }) == SSW_ERR_BAD_ARG);
    REQUIRE(status_of([&] { wm::collude(ctx, {}, {}); }) == SSW_ERR_BAD_ARG && status_of([&] { wm::jpeg(ctx, {}, {}); }) == SSW_ERR_BAD_ARG);   // empty frames
    REQUIRE(status_of([&] { wm::filter(ctx, {}, {}); }) == SSW_ERR_BAD_ARG && status_of([&] { wm::scale_attack(ctx, {}, {}); }) == SSW_ERR_BAD_ARG);
    REQUIRE(status_of([&] { wm::resample(ctx, {}, 4, 4); }) == SSW_ERR_BAD_ARG && status_of([&] { wm::affine(ctx, {}, 4, 4, wm::Matrix{}); }) == SSW_ERR_BAD_ARG);
    REQUIRE(status_of([&] { wm::rotate(ctx, {}, 1.0); }) == SSW_ERR_BAD_ARG && status_of([&] { wm::unrotate(ctx, good, {&good}, {}); }) == SSW_ERR_BAD_ARG);
    REQUIRE(status_of([&] { wm::mark_many(ctx, {}, {}); }) == SSW_ERR_BAD_ARG && status_of([&] { wm::mark_many(ctx, {&good, &good}, {&m0}); }) == SSW_ERR_BAD_ARG);
    REQUIRE(status_of([&] { wm::mark_many(ctx, {&good, &wide}, {&m0, &m0}); }) == SSW_ERR_BAD_DIMS);
    REQUIRE(status_of([&] { wm::mark_many(ctx, {&good, &good}, {&m0, &longer}); }) == SSW_ERR_LENGTH_MISMATCH);
    REQUIRE(status_of([&] { wm::extract_many(ctx, {}, {}, K, {}); }) == SSW_ERR_BAD_ARG);
    REQUIRE(status_of([&] { wm::extract_many(ctx, {&good}, {&good, &good}, K, {}); }) == SSW_ERR_BAD_ARG);
    REQUIRE(status_of([&] { wm::extract_many(ctx, {&good}, {&good}, K, {&m0, &m0}); }) == SSW_ERR_BAD_ARG);
    REQUIRE(status_of([&] { wm::extract_many(ctx, {&good, &good}, {&good, &wide}, K, {}); }) == SSW_ERR_BAD_DIMS);
    REQUIRE(status_of([&] { wm::extract_many(ctx, {&good}, {&good}, K, {&longer}); }) == SSW_ERR_LENGTH_MISMATCH);
    REQUIRE(ssw_stub_calls() == made);
    // frames of unequal size in the calls that copy frames to the device: thrown between library calls, nothing may stay behind
    REQUIRE(status_of([&] { wm::quality(ctx, good, {&good, &wide}); }) == SSW_ERR_BAD_DIMS && status_of([&] { wm::ssim(ctx, good, {&bad8}); }) == SSW_ERR_BAD_DIMS);
    REQUIRE(status_of([&] { wm::collude(ctx, {&good, &wide}, {{SSW_COLLUDE_MIN, {0}}}); }) == SSW_ERR_BAD_DIMS);
    REQUIRE(status_of([&] { wm::jpeg(ctx, {&good, &wide}, {{0, 50}, {1, 50}}); }) == SSW_ERR_BAD_DIMS);
    REQUIRE(status_of([&] { wm::filter(ctx, {&good, &wide}, {wm::FilterJob::median(0)}); }) == SSW_ERR_BAD_DIMS);
    REQUIRE(status_of([&] { wm::scale_attack(ctx, {&good, &wide}, {wm::Scale{0, 4, 4}}); }) == SSW_ERR_BAD_DIMS);
    REQUIRE(status_of([&] { wm::resample(ctx, {&good, &wide}, 4, 4); }) == SSW_ERR_BAD_DIMS);
    REQUIRE(status_of([&] { wm::affine(ctx, {&good, &wide}, 4, 4, wm::Matrix{1, 0, 0, 0, 1, 0}); }) == SSW_ERR_BAD_DIMS);
    REQUIRE(status_of([&] { wm::rotate(ctx, {&good, &wide}, 1.0); }) == SSW_ERR_BAD_DIMS);
    REQUIRE(status_of([&] { wm::rotate_attack(ctx, good, {&good, &wide}, {wm::Rotate{0, 1.0}}); }) == SSW_ERR_BAD_DIMS);
    REQUIRE(status_of([&] { wm::rotate_attack(ctx, bad8, {&good}, {wm::Rotate{0, 1.0}}); }) == SSW_ERR_BAD_DIMS);
    REQUIRE(status_of([&] { wm::unrotate(ctx, good, {&good, &wide}, {1.0, 2.0}); }) == SSW_ERR_BAD_DIMS);
    size_t live[5];
    ssw_stub_live(live);
    REQUIRE(live[0] == 0 && live[1] == 0 && live[2] == 1 && live[3] == 1 && live[4] == 1);
    // a status the library answers is the one the wrapper throws
    (void)w.result();
    REQUIRE(status_of([&] { (void)w.result(); }) == SSW_ERR_CONSUMED);
    wm::Catalogue cat(ctx);
    const wm::ImageRgb8 big = image<wm::ImageRgb8>(40, 36, 30);
    const std::vector<float> ext(K, 1.f);
    REQUIRE(status_of([&] { wm::Tester(ctx, ext).similarity(longer); }) == SSW_ERR_LENGTH_MISMATCH);
    REQUIRE(status_of([&] { cat.match({big}, 9); }) == SSW_ERR_BAD_ARG && status_of([&] { wm::signature(ctx, {tiny}); }) == SSW_ERR_BAD_ARG);
    REQUIRE(status_of([&] { wm::locate(ctx, good, {good}, {wm::Placement{0, 0, W + 1, H}}); }) == SSW_ERR_BAD_ARG);
    REQUIRE(status_of([&] { wm::locate_scaled(ctx, wide, {good}, {wm::ScaleRange{16, 40}}); }) == SSW_ERR_BAD_ARG);
    ssw_stub_live(live);
    REQUIRE(live[0] == 0);
}

// ---- the failure sweep -------------------------------------------------------------------------------------------------------------
size_t sweep(const char* name, const std::function<void()>& flow) {
    REQUIRE(nothing_live());
    const size_t start = ssw_stub_calls();
    flow();
    const size_t calls = ssw_stub_calls() - start;
    REQUIRE(calls > 0 && nothing_live());
    size_t visited = 0;
    for (size_t n = 1; n <= calls; ++n) {
        const size_t from = ssw_stub_calls();
        ssw_stub_fail_at(n, SSW_ERR_OUT_OF_MEMORY);
        int status = SSW_OK;
        try {
            flow();
        } catch (const wm::Error& e) {
            status = e.status();
        }
        ssw_stub_fail_at(0, SSW_OK);
        if (status != SSW_ERR_OUT_OF_MEMORY || ssw_stub_calls() - from != n || !nothing_live()) {
            size_t live[5];
            ssw_stub_live(live);
            std::fprintf(stderr, "sweep %s: call %zu of %zu: status %d after %zu calls, live %zu %zu %zu %zu %zu\n", name, n, calls, status,
                         ssw_stub_calls() - from, live[0], live[1], live[2], live[3], live[4]);
            std::exit(1);
        }
        ++visited;
    }
    REQUIRE(visited == calls);
    std::printf("sweep %s %zu\n", name, calls);
    return calls;
}
}  // namespace

int main() {
    basics();
    const std::pair<const char*, std::function<void()>> flows[] = {
        {"context", context},
        {"writer32f", writer<wm::ImageRgb32F>}, {"writer8", writer<wm::ImageRgb8>}, {"writer16", writer<wm::ImageRgb16>},
        {"reader32f", reader<wm::ImageRgb32F>}, {"reader8", reader<wm::ImageRgb8>}, {"reader16", reader<wm::ImageRgb16>},
        {"trace", trace}, {"locate", locate}, {"locate_scaled", locate_scaled}, {"catalogue", catalogue}, {"strength", strength},
        {"rotation", rotation}, {"many", many},
    };
    size_t total = 0;
    for (const auto& f : flows) total += sweep(f.first, f.second);
    header_checks();
    REQUIRE(nothing_live());
    std::printf("calls swept %zu\nok\n", total);
    return 0;
}
