// Runs the forensic wrappers of include/ssw.hpp against the real library on files that tests/test_cpp_forensic_gpu.py wrote, and
// writes what they return; the test compares it with the Python wrappers' answers on the same inputs, exactly.
//   forensic_wrappers_test <in_dir> <out_dir>
// Wrappers run: Writer::mark_copies / mark_copies_rgb8 (the writer stays usable), both Reader::trace overloads, Placement::whole_frame,
// Suspect from ImageRgba8, locate, locate_scaled, signature, Catalogue, mark_many, extract_many, ImageRgb16 through Writer, Reader::base
// and ReaderDerived, PinnedBuffer, Context::transfer_stats; and five error paths of the real library.
// in_dir (raw arrays; the frame B is 192 x 128): B.u8 B32.f32 marks.f32 [4][64] small.u8 (96 x 64) cut_rgba.u8 (80 x 64 x 4)
//   rect.u8 (80 x 64) cut60.u8 (60 x 48) noise.u8 (33 x 35) rolled.u8 flipped.u8 sub0.u8 sub1.u8 sub2.u8 (96 x 64) marked16.u16
// out_dir: raw result files, named below.  stdout: one line per record, "ok" last.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>

#include "ssw.hpp"

namespace {
constexpr size_t W = 192, H = 128, K = 64, SW = 96, SH = 64, SK = 32;
std::string in_dir, out_dir;

template <class T> std::vector<T> read(const std::string& name, size_t n) {
    std::vector<T> v(n);
    std::ifstream f(in_dir + "/" + name, std::ios::binary);
    f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(n * sizeof(T)));
    if (!f || f.peek() != EOF) throw std::runtime_error("cannot read " + name);
    return v;
}
template <class Img> Img image(const std::string& name, size_t w, size_t h, size_t channels = 3) {
    Img im(w, h);
    im.data = read<typename decltype(im.data)::value_type>(name, w * h * channels);
    return im;
}
struct Out {
    std::ofstream f;
    explicit Out(const std::string& name) : f(out_dir + "/" + name, std::ios::binary) {}
    template <class T> void put(const std::vector<T>& v) { f.write(reinterpret_cast<const char*>(v.data()), (std::streamsize)(v.size() * sizeof(T))); }
    ~Out() { if (!f) std::fprintf(stderr, "a result file could not be written\n"); }
};
void put_trace(const std::string& prefix, const wm::TraceResult& r) {
    Out ext(prefix + "_ext.f32"), sims(prefix + "_sims.f32"), best(prefix + "_best.u32"), best_sim(prefix + "_best_sim.f32"), n_exceed(prefix + "_n_exceed.u32");
    for (const auto& e : r.extracted) ext.put(e);
    for (const auto& s : r.sims) sims.put(s);
    best.put(r.best); best_sim.put(r.best_sim); n_exceed.put(r.n_exceed);
}
void put_located(const char* what, const std::vector<wm::Located>& found) {
    for (const wm::Located& l : found)
        std::printf("%s %zu %zu %zu %zu %llu %a\n", what, l.placement.x, l.placement.y, l.placement.w, l.placement.h, (unsigned long long)l.sad, l.mean_abs_diff);
}
void put_matches(const char* what, const std::vector<std::vector<wm::Catalogue::Match>>& m) {
    for (size_t s = 0; s < m.size(); ++s)
        for (size_t t = 0; t < m[s].size(); ++t) std::printf("%s %zu %zu %u %u\n", what, s, t, m[s][t].index, m[s][t].distance);
}
template <class F> void put_error(const char* what, F f) {
    int status = SSW_OK;
    try { f(); } catch (const wm::Error& e) { status = e.status(); }
    std::printf("error %s %d\n", what, status);
}
}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    in_dir = argv[1]; out_dir = argv[2];
    try {
        wm::Context ctx(0);
        const wm::ImageRgb8 B = image<wm::ImageRgb8>("B.u8", W, H);
        const wm::ImageRgb32F B32 = image<wm::ImageRgb32F>("B32.f32", W, H);
        const std::vector<float> all = read<float>("marks.f32", 4 * K);
        std::vector<wm::MarkBuf> marks, short_marks;
        for (size_t i = 0; i < 4; ++i) marks.push_back(wm::MarkBuf::from(all.data() + i * K, K));
        for (size_t i = 0; i < 3; ++i) short_marks.push_back(wm::MarkBuf::from(all.data() + i * K, SK));
        const std::vector<const wm::MarkBuf*> mp{&marks[0], &marks[1], &marks[2], &marks[3]}, smp{&short_marks[0], &short_marks[1], &short_marks[2]};

        // 1. fingerprinting; the writer is still usable afterwards
        std::vector<wm::ImageRgb8> copies;
        {
            wm::Writer writer(ctx, B);
            copies = writer.mark_copies_rgb8(mp);
            Out c8("copies8.u8"), again("again8.u8"), c32("copies32.f32");
            for (const wm::ImageRgb8& c : copies) c8.put(c.data);
            again.put(writer.mark_rgb8({&marks[0]}).data);
            wm::Writer writer32(ctx, B32);
            for (const wm::ImageRgb32F& c : writer32.mark_copies(mp)) c32.put(c.data);
        }
        if (copies.size() != 4) return 3;
        // 2. plain trace: the four copies and the original itself
        const wm::Reader base = wm::Reader::base(ctx, B);
        put_trace("plain", base.trace({&copies[0], &copies[1], &copies[2], &copies[3], &B}, mp));
        // 3. restoring trace: a copy as it is, a scaled copy, an RGBA cut-out with a transparent border
        const wm::ImageRgb8 small = image<wm::ImageRgb8>("small.u8", SW, SH), rect = image<wm::ImageRgb8>("rect.u8", 80, 64),
                            cut60 = image<wm::ImageRgb8>("cut60.u8", 60, 48), noise = image<wm::ImageRgb8>("noise.u8", 33, 35);
        const wm::ImageRgba8 cut = image<wm::ImageRgba8>("cut_rgba.u8", 80, 64, 4);
        put_trace("restored", base.trace(B, {copies[1], small, cut}, {wm::Placement::whole_frame(B), wm::Placement::whole_frame(B), wm::Placement{40, 24, 0, 0}}, mp));
        // 4. locate: the exact rectangle at its own size, the scaled one at the size it had
        put_located("locate_own", wm::locate(ctx, B, {rect}));
        put_located("locate_sized", wm::locate(ctx, B, {cut60}, {wm::Placement{0, 0, 80, 64}}));
        // 5. the scale ladder
        put_located("locate_scaled", wm::locate_scaled(ctx, B, {cut60}, {wm::ScaleRange{64, 96}}));
        // 6. signatures of three images of three sizes, one of them RGBA
        {
            Out sigs("sigs.u8");
            for (const auto& s : wm::signature(ctx, {B, cut, noise})) sigs.put(std::vector<uint8_t>(s.begin(), s.end()));
        }
        // 7. the catalogue: three entries, two suspects, top 1 and top 8; a fourth entry, and again
        {
            const wm::ImageRgb8 rolled = image<wm::ImageRgb8>("rolled.u8", W, H), flipped = image<wm::ImageRgb8>("flipped.u8", W, H);
            wm::Catalogue cat(ctx);
            cat.add("B", B); cat.add("rolled", rolled); cat.add("flipped", flipped);
            put_matches("match1", cat.match({copies[1], rolled}));
            put_matches("match8", cat.match({copies[1], rolled}, 8));
            cat.add("small", small);
            put_matches("match8_four", cat.match({copies[1], rolled}, 8));
            std::printf("catalogue %zu %s\n", cat.size(), cat.name(3).c_str());
            put_error("match_top9", [&] { cat.match({rolled}, 9); });
        }
        // 8. the streaming calls
        {
            const wm::ImageRgb8 s0 = image<wm::ImageRgb8>("sub0.u8", SW, SH), s1 = image<wm::ImageRgb8>("sub1.u8", SW, SH), s2 = image<wm::ImageRgb8>("sub2.u8", SW, SH);
            const std::vector<wm::ImageRgb8> marked = wm::mark_many(ctx, {&s0, &s1, &s2}, smp);
            if (marked.size() != 3) return 3;
            Out m8("many8.u8"), ext("many_ext.f32"), sims("many_sims.f32"), ext_only("many_ext_only.f32");
            for (const wm::ImageRgb8& m : marked) m8.put(m.data);
            const wm::ExtractedMany with = wm::extract_many(ctx, {&s0, &s1, &s2}, {&marked[0], &marked[1], &marked[2]}, SK, smp);
            const wm::ExtractedMany without = wm::extract_many(ctx, {&s0, &s1, &s2}, {&marked[0], &marked[1], &marked[2]}, SK, {});
            for (const auto& e : with.extracted) ext.put(e);
            sims.put(with.similarity);
            for (const auto& e : without.extracted) ext_only.put(e);
            std::printf("many %zu %zu %zu %zu\n", with.extracted.size(), with.similarity.size(), without.extracted.size(), without.similarity.size());
        }
        // 9. a 16-bit original: marked, and read again
        {
            wm::ImageRgb16 B16(W, H);
            for (size_t i = 0; i < B16.data.size(); ++i) B16.data[i] = (uint16_t)(B.data[i] * 257);
            Out marked("marked16.f32"), ext("ext16.f32");
            marked.put(wm::Writer(ctx, B16).mark({&marks[0]}).data);
            const wm::ImageRgb16 marked16 = image<wm::ImageRgb16>("marked16.u16", W, H);
            std::vector<float> e(K);
            wm::Reader::base(ctx, B16).extract(wm::ReaderDerived(ctx, marked16), e);
            ext.put(e);
        }
        // 10. pinned memory and the transfer counters
        {
            wm::PinnedBuffer pinned(ctx, 1 << 20);
            uint8_t* p = static_cast<uint8_t*>(pinned.data());
            for (size_t i = 0; i < pinned.size(); ++i) p[i] = (uint8_t)(i * 13);
            size_t wrong = 0;
            for (size_t i = 0; i < pinned.size(); ++i) wrong += p[i] != (uint8_t)(i * 13);
            std::printf("pinned %zu %zu\n", pinned.size(), wrong);
        }
        std::printf("transfer_stats %zu\n", ctx.transfer_stats(true).size());
        // the real library's error paths, as wm::Error
        put_error("trace_other_size", [&] { base.trace({&small}, mp); });
        put_error("result_twice", [&] {
            wm::Writer w(ctx, B);
            (void)w.result();
            (void)w.result();
        });
        put_error("locate_too_large", [&] { wm::locate(ctx, B, {rect}, {wm::Placement{0, 0, W + 1, H}}); });
        put_error("locate_scaled_below_32", [&] { wm::locate_scaled(ctx, B, {cut60}, {wm::ScaleRange{16, 96}}); });
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
